#!/usr/bin/env python
"""What one tick of the streaming batch (`pantomatrix_amd.streaming.StreamBatch`) costs on the MI355X at S = 1, 8, 32 and 64 slots, all of
them live and one window behind their audio — every tick each session pushes the 32 000 samples of its next window and the batch steps:
  replay     `step()` of a captured batch: staging on the host, two host-to-device copies, ONE graph replay, one device-to-host copy;
  eager      the same tick, its launches issued one by one (use_graph=False);
  separate   S separate B = 1 windows — `EmageAudioModel._window_step` (forward, codes, seed decode) and a
             `decode(get_global_motion=True)` of the last 116 codes per session — which is what serving S live sessions costs without this
             module (a server there would in fact decode each session's whole history; the arm does not charge for that).
`decode_ms` is the eager segment decode + emit alone (`_decode_segments` at B = S, T = 60 + 2 lag, and `emage_stream_emit`), and
`decode_share_of_eager_tick` its share of the eager tick — a share of the replay is not measured here (it needs a kernel trace).
Wall time per tick around work that ends in a device synchronise (`step()` ends in one); the arms alternate, `--runs` times each, and the
median and the run-to-run spread are reported.  Writes one JSON document to `--out` and prints it.
`--audio-input RATE:CH:FMT` measures something else: the captured tick of a batch built with `audio_inputs=(that input,)` — raw PCM staged,
`stream_push_resample` as the first launch — against the captured 16 kHz f32 tick of the same tree, the two interleaved on the same device,
into profiles/stream_resample_bench.json.  The kernel's own time needs a kernel trace of such a run (`rocprofv3 --kernel-trace --stats`).
`--hints` measures a third thing: the captured tick of a batch built with `motion_hints=True` whose every session is hinted (upper body kept,
60 hint frames staged per slot and tick: `stream_push_hints`, `pack_motion_hints`) against the captured tick without hints, interleaved, with
the staged bytes per tick, into profiles/stream_hints_bench.json.  The difference holds host staging and the launch alike; their split needs
a kernel trace taken in a run of its own."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HOP_SAMPLES = 32000                                      # rule 1: a session's need grows by 60 frames = 32 000 samples a window


def summary(values):
    return {"runs": [round(v, 3) for v in values], "median": round(float(np.median(values)), 3), "spread": round(max(values) - min(values), 3)}


class Live:
    """S sessions of one batch, fed from one long waveform that each slot enters at another sample."""

    def __init__(self, sb, base):
        from pantomatrix_amd import streaming
        self.sb, self.waves = sb, [base[1009 * k:] for k in range(sb.slots)]
        self.sessions = [sb.open() for _ in range(sb.slots)]
        for s, w in zip(self.sessions, self.waves):
            s.push(w[:streaming.window_need(0)])
        assert len(sb.step()) == sb.slots

    def tick(self):
        from pantomatrix_amd import streaming
        for s, w in zip(self.sessions, self.waves):
            s.push(w[s.pushed:streaming.window_need(s.windows)])
        out = self.sb.step()
        assert len(out) == self.sb.slots and all(e.poses.shape[0] == 60 for e in out.values())


class LiveRaw:
    """`Live` for a batch that resamples: S sessions fed raw PCM of one `AudioInput`, each tick the frames that make the next window final."""

    def __init__(self, sb, base, inp):
        from pantomatrix_amd import audio, streaming
        self.sb, (self.up, self.down) = sb, audio.rate_ratio(inp.rate, 16000)
        self.half = audio.stream_half(self.up, self.down)
        t = np.arange(int((len(base) - 1) * self.down / self.up)) * (self.up / self.down)          # the 16 kHz waveform, linearly interpolated to the rate
        x = np.interp(t, np.arange(len(base)), base).astype(np.float32)
        if inp.fmt == "f32":
            pcm = x[:, None]
        elif inp.fmt == "s16":
            pcm = np.round(x * 32767.0).clip(-32768, 32767).astype(np.int16)[:, None]
        elif inp.fmt == "s32":
            pcm = np.round(x.astype(np.float64) * (2.0 ** 31 - 1)).astype(np.int64).clip(-2 ** 31, 2 ** 31 - 1).astype(np.int32)[:, None]
        else:
            v = np.round(x * 8388607.0).astype(np.int64) & 0xFFFFFF
            pcm = np.stack([v & 0xFF, (v >> 8) & 0xFF, (v >> 16) & 0xFF], axis=-1).astype(np.uint8)[:, None, :]
        pcm = np.repeat(pcm, inp.channels, axis=1).reshape(len(x), -1)                               # every channel the same signal
        skip = 1009 * self.down // self.up
        self.waves = [pcm[skip * k:] for k in range(sb.slots)]
        self.sessions = [sb.open() for _ in range(sb.slots)]
        self.frames_per_tick = 0
        self.tick(first=streaming.window_need(0))

    def frames_for(self, need):
        """The fewest frames whose FINAL outputs reach `need` samples: n up - half > (need - 1) down."""
        return ((need - 1) * self.down + self.half) // self.up + 1

    def tick(self, first=None):
        from pantomatrix_amd import streaming
        for s, w in zip(self.sessions, self.waves):
            upto = self.frames_for(first or streaming.window_need(s.windows))
            self.frames_per_tick = upto - s.frames_in
            s.push(w[s.frames_in:upto])
        out = self.sb.step()
        assert len(out) == self.sb.slots and (first or all(e.poses.shape[0] == 60 for e in out.values()))


def resample_arm(args, inp):
    """`--audio-input`: the captured tick with that input against the 16 kHz f32 tick of the same tree, interleaved on the same device."""
    from pantomatrix_amd import streaming, synthetic
    from tools import workloads
    model, vq = workloads.product_models(precision=args.precision, device="cuda")
    ticks = 2 + args.runs * (args.steps + 1)
    seconds = (ticks + 2) * HOP_SAMPLES // 16000 + 4
    base = synthetic.synthetic_audio(1, seconds * 16000 + 1009 * max(args.slots))[0].numpy()
    parent = {}
    try:
        with open(os.path.join(ROOT, "profiles", "stream_bench.json")) as f:
            parent = {k: v["tick_ms"]["replay"] for k, v in json.load(f)["slots"].items()}
    except (OSError, KeyError, ValueError):
        pass
    result = {"what": f"one captured tick of StreamBatch, every slot live, fed {inp} (stream_push_resample) vs fed 16 kHz f32 (stream_push): same tree, "
                      "arms interleaved; parent_replay_tick_ms is the replay tick recorded in profiles/stream_bench.json",
              "commit": args.commit, "audio_input": {"rate": inp.rate, "channels": inp.channels, "fmt": inp.fmt},
              "config": {"precision": args.precision, "ticks_per_run": args.steps, "runs": args.runs, "samples_per_slot_and_tick": HOP_SAMPLES}, "slots": {}}
    for n in args.slots:
        live = {"f32_16k": Live(streaming.StreamBatch(model, vq, slots=n, max_seconds=seconds, use_graph=True), base),
                "resample": LiveRaw(streaming.StreamBatch(model, vq, slots=n, max_seconds=seconds, use_graph=True, audio_inputs=(inp,)), base, inp)}
        ms = {k: [] for k in live}
        for _ in range(args.runs):
            for name, l in live.items():
                l.tick()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    l.tick()
                torch.cuda.synchronize()
                ms[name].append(1e3 * (time.perf_counter() - t0) / args.steps)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        sb = live["resample"].sb
        result["slots"][str(n)] = {"tick_ms": {k: summary(v) for k, v in ms.items()}, "resample_minus_f32_ms": round(med["resample"] - med["f32_16k"], 3),
                                   "resample_over_f32": round(med["resample"] / med["f32_16k"], 3), "parent_replay_tick_ms": parent.get(str(n)),
                                   "frames_per_slot_and_tick": live["resample"].frames_per_tick,
                                   "staged_bytes_per_tick": n * live["resample"].frames_per_tick * sb.frame_bytes[0], "history_frames": sb.hist_len}
        for l in live.values():
            for s in l.sessions:
                s._staged, s.closed = [], True                              # dropped, not closed: the tail of a benchmark session is nobody's output
        del live, sb
        torch.cuda.empty_cache()
    return result


class LiveHinted(Live):
    """`Live` in a batch built with motion_hints=True: every session is hinted — the upper body kept from a 'capture' — and pushes the 60 hint
    frames of its next window with the window's audio, every tick."""

    def __init__(self, sb, base):
        from pantomatrix_amd.recordings import identity_seed, part_columns
        self.sb, self.waves = sb, [base[1009 * k:] for k in range(sb.slots)]
        g = np.random.default_rng(0)
        self.motion = identity_seed(1, 64)[0].numpy() + (0.05 * g.standard_normal((64, 337))).astype(np.float32)
        self.mask = np.ones((64, 337), np.uint8)
        self.mask[:, part_columns("upper")] = 0
        self.sessions = [sb.open(motion=True) for _ in range(sb.slots)]
        self.tick(first=True)

    def tick(self, first=False):
        from pantomatrix_amd import streaming
        n = 64 if first else 60
        for s, w in zip(self.sessions, self.waves):
            s.push(w[s.pushed:streaming.window_need(s.windows)])
            s.push_motion(self.motion[:n], self.mask[:n])
        out = self.sb.step()
        assert len(out) == self.sb.slots and (first or all(e.poses.shape[0] == 60 for e in out.values()))


def hints_arm(args):
    """`--hints`: the captured tick of a batch whose every slot is hinted (upper body kept, 60 hint frames pushed per slot and tick) against
    the captured tick of a batch without motion hints, same tree, the two interleaved on the same device."""
    from pantomatrix_amd import streaming, synthetic
    from tools import workloads
    model, vq = workloads.product_models(precision=args.precision, device="cuda")
    ticks = 2 + args.runs * (args.steps + 1)
    seconds = (ticks + 2) * HOP_SAMPLES // 16000 + 4
    base = synthetic.synthetic_audio(1, seconds * 16000 + 1009 * max(args.slots))[0].numpy()
    result = {"what": "one captured tick of StreamBatch, every slot live: every session hinted (motion_hints=True; upper body kept, 60 hint frames "
                      "staged per slot and tick, stream_push_hints + pack_motion_hints) vs a batch without motion hints; same tree, arms interleaved",
              "commit": args.commit,
              "config": {"precision": args.precision, "ticks_per_run": args.steps, "runs": args.runs, "samples_per_slot_and_tick": HOP_SAMPLES,
                         "hint_frames_per_slot_and_tick": 60}, "slots": {}}
    for n in args.slots:
        live = {"plain": Live(streaming.StreamBatch(model, vq, slots=n, max_seconds=seconds, use_graph=True), base),
                "hinted": LiveHinted(streaming.StreamBatch(model, vq, slots=n, max_seconds=seconds, use_graph=True, motion_hints=True), base)}
        ms = {k: [] for k in live}
        for _ in range(args.runs):
            for name, l in live.items():
                l.tick()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    l.tick()
                torch.cuda.synchronize()
                ms[name].append(1e3 * (time.perf_counter() - t0) / args.steps)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        sb = live["hinted"].sb
        result["slots"][str(n)] = {"tick_ms": {k: summary(v) for k, v in ms.items()}, "hinted_minus_plain_ms": round(med["hinted"] - med["plain"], 3),
                                   "hinted_over_plain": round(med["hinted"] / med["plain"], 3), "staged_hint_bytes_per_tick": sb.hint_bytes_staged,
                                   "hint_ring_rows": sb.hint_rows, "hint_ring_bytes_per_slot": (sb.hint_rows + 4) * 344 * 5}
        for l in live.values():
            for s in l.sessions:
                s._staged, s._hint_staged, s.closed = [], [], True           # dropped, not closed: the tail of a benchmark session is nobody's output
        del live, sb
        torch.cuda.empty_cache()
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, nargs="+", default=[1, 8, 32, 64])
    ap.add_argument("--steps", type=int, default=40, help="ticks per timed run")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--out", default=None, help="default: profiles/stream_bench.json, or profiles/stream_resample_bench.json with --audio-input")
    ap.add_argument("--commit", default=None, help="recorded in the document (the measured tree is not always a git checkout)")
    ap.add_argument("--audio-input", default=None, metavar="RATE:CH:FMT", help="measure the resampling tick for this input (e.g. 44100:2:s16) "
                    "against the 16 kHz f32 tick instead of the three arms above")
    ap.add_argument("--hints", action="store_true", help="measure the tick of a batch whose every session pushes motion hints against the tick "
                    "without hints instead of the three arms above (profiles/stream_hints_bench.json)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_stream needs an MI355X: none of its figures means anything on a CPU"
    if args.hints:
        result = hints_arm(args)
        result["peak_memory_gb"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
        out = args.out or os.path.join(ROOT, "profiles", "stream_hints_bench.json")
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps(result))
        return
    if args.audio_input:
        from pantomatrix_amd.audio import AudioInput
        rate, ch, fmt = args.audio_input.split(":")
        result = resample_arm(args, AudioInput(int(rate), int(ch), fmt))
        result["peak_memory_gb"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
        out = args.out or os.path.join(ROOT, "profiles", "stream_resample_bench.json")
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps(result))
        return
    args.out = args.out or os.path.join(ROOT, "profiles", "stream_bench.json")
    from pantomatrix_amd import ops, streaming, synthetic
    from pantomatrix_amd.recordings import identity_seed
    from tools import workloads
    dev = "cuda"
    model, vq = workloads.product_models(precision=args.precision, device=dev)
    ticks = 2 + args.runs * (args.steps + 1)
    seconds = (ticks + 2) * HOP_SAMPLES // 16000 + 4
    base = synthetic.synthetic_audio(1, seconds * 16000 + 1009 * max(args.slots))[0].numpy()
    result = {"what": "one tick of StreamBatch, every slot live: graph replay vs eager tick vs S separate B = 1 windows (the parent commit's serving cost)",
              "commit": args.commit, "config": {"precision": args.precision, "ticks_per_run": args.steps, "runs": args.runs, "samples_pushed_per_slot_and_tick": HOP_SAMPLES},
              "slots": {}}
    for n in args.slots:
        live = {"replay": Live(streaming.StreamBatch(model, vq, slots=n, max_seconds=seconds, use_graph=True), base),
                "eager": Live(streaming.StreamBatch(model, vq, slots=n, max_seconds=seconds, use_graph=False), base)}
        sb = live["eager"].sb
        lag, seg_len = sb.lag, sb.seg_len
        audio = torch.from_numpy(base[:64 * 533].copy()).to(dev)[None]
        spk, seed1 = torch.zeros(1, 1, dtype=torch.long, device=dev), identity_seed(1).to(dev)
        motion, mask = identity_seed(1, 64).to(dev), torch.ones(1, 64, 337, device=dev)
        codes = {p: torch.zeros(1, 64, dtype=torch.int64, device=dev) for p in sb.parts}
        seg = {f"{p}_index": torch.zeros(1, seg_len, dtype=torch.int64, device=dev) for p in sb.parts}
        carry = sb.carry.clone()                                             # the decode arm must not move the live sessions' translation

        def separate():
            for _ in range(n):
                model._window_step(vq, audio, spk, motion, mask, seed1, codes, 0, True)
                pred = vq.decode(**seg, get_global_motion=True, ref_trans=torch.zeros(1, 3, device=dev))
                pred["trans"].cpu()                                          # a session's frames leave the device every window
            torch.cuda.synchronize()

        def decode():
            aa, expr, vel = vq._decode_segments(**{f"{p}_index": v for p, v in sb._codes_of(sb.segment).items()})
            v = sb.out_views
            ops.stream_emit(sb.table, aa, expr, vel, 54, 1 / 30, sb.segment, carry, v["poses"], v["expressions"], v["trans"], v["codes"], sb.status)
            torch.cuda.synchronize()

        arms = {"replay": live["replay"].tick, "eager": live["eager"].tick, "separate": separate, "decode": decode}
        ms = {k: [] for k in arms}
        for _ in range(args.runs):
            for name, fn in arms.items():
                steps = args.steps if name != "separate" else max(2, args.steps * 8 // max(n, 8))
                fn()                                                         # warm-up of the arm's shapes (and of the caches behind the other arms)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    fn()
                torch.cuda.synchronize()
                ms[name].append(1e3 * (time.perf_counter() - t0) / steps)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        result["slots"][str(n)] = {
            "tick_ms": {k: summary(ms[k]) for k in ("replay", "eager", "separate")}, "decode_ms": summary(ms["decode"]),
            "decode_share_of_eager_tick": round(med["decode"] / med["eager"], 3), "replay_over_eager": round(med["replay"] / med["eager"], 3),
            "replay_over_separate": round(med["replay"] / med["separate"], 3), "frames_per_second_replay": round(n * 60 / (med["replay"] * 1e-3), 1),
            "real_time_sessions_replay": round(n * 2000.0 / med["replay"], 1), "lag_frames": lag, "segment_rows": seg_len,
            "ring_samples_per_slot": sb.ring_len}
        for l in live.values():
            for s in l.sessions:
                s._staged, s.closed = [], True                              # dropped, not closed: the tail of a benchmark session is nobody's output
        del live, sb
        torch.cuda.empty_cache()
    result["peak_memory_gb"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
