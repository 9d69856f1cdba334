#!/usr/bin/env python
"""What feeding the EMAGE training step costs on the MI355X, at BASELINE config 3 (56 clips of 64 frames per GPU) over a synthetic clip store
of BEAT2 speaker-2 size (~190 k frames: ~200 MB of motion, ~200 MB of 16 kHz s16 audio, resident on the device):
  fill          `data.ClipLoader.fill()`: emage_gather_clips + emage_motion_mask + the counter update, device time per call;
  host_path     the same batch by the host: `ClipStore.gather_host` into pinned staging buffers, the five host-to-device copies, and the
                reference's `torch.rand(bs, t, 337) < r` with its copy (train_emage_audio.py:163-165), wall time per batch up to a synchronise;
  step_static   `Trainer.capture(batch, mask)` on static buffers, ms per `replay()` (the step as it was before the loader existed);
  step_loader   `Trainer.capture(loader.batch, loader.random_mask, prologue=loader.fill)`, ms per `replay()`;
  step_static_twin   a second trainer captured like step_static on its own model and buffers: what two captures of the SAME step differ by.
Every figure is taken `--runs` times (the captured steps alternate), and the run-to-run spread is reported with it.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def synthetic_store(total_frames, n_recordings, clip, stride, device, seed=0):
    from pantomatrix_amd import data
    rng = np.random.default_rng(seed)
    f = total_frames // n_recordings
    spf = data.samples_per_frame(16000)
    recordings = []
    for _ in range(n_recordings):
        recordings.append(dict(poses=(0.3 * rng.standard_normal((f, 165), dtype=np.float32)), expressions=(0.5 * rng.standard_normal((f, 100), dtype=np.float32)),
                               trans=(0.1 * rng.standard_normal((f, 3), dtype=np.float32)), foot_contact=rng.integers(0, 2, (f, 4)).astype(np.float32),
                               audio=rng.integers(-3276, 3277, f * spf + 7).astype(np.int16)))
    clips = [(r, s, s + clip) for r in range(n_recordings) for s in range(0, f - clip + 1, stride)]
    return data.ClipStore.from_arrays(recordings, clips, device)


def summary(values):
    return {"runs": [round(v, 4) for v in values], "median": round(float(np.median(values)), 4), "spread": round(max(values) - min(values), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=56)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--total-frames", type=int, default=190000)
    ap.add_argument("--recordings", type=int, default=25)
    ap.add_argument("--stride", type=int, default=20)
    ap.add_argument("--steps", type=int, default=40, help="replays per run of a captured step")
    ap.add_argument("--fills", type=int, default=200, help="fill() calls / host batches per run")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--no-step", action="store_true", help="loader figures only")
    ap.add_argument("--commit", default=None, help="recorded in the line (the measured tree is not always a git checkout)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_clip_loader needs an MI355X: none of its figures means anything on a CPU"
    from pantomatrix_amd import data, training
    from tools import workloads
    dev = "cuda"
    t0 = time.perf_counter()
    store = synthetic_store(args.total_frames, args.recordings, args.frames, args.stride, dev)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    loader = data.ClipLoader(store, args.batch, mask_seed=1)
    b, t = args.batch, args.frames
    line = {"what": "device-resident clip store: ClipLoader.fill() vs the host path, and the captured training step with and without the loader as its prologue",
            "commit": args.commit, "config": {"clips_per_gpu": b, "frames_per_clip": t, "store_frames": store.total_frames, "store_clips": store.n_clips,
                                              "batches_per_epoch": len(loader), "audio_format": store.audio_format, "precision": args.precision},
            "store_build_s": round(build_s, 2),
            "store_device_mb": round(sum(v.numel() * v.element_size() for v in store.arrays.values()) / 2 ** 20, 1)}

    # ---- fill(): device time per call (events around a run of calls; the launches queue up, so this is the device's time, not the host's)
    for _ in range(10):
        loader.fill()
    torch.cuda.synchronize()
    fill_ms = []
    for _ in range(args.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.fills):
            loader.fill()
        e1.record()
        torch.cuda.synchronize()
        fill_ms.append(e0.elapsed_time(e1) / args.fills)
    loader.check()
    line["fill_ms"] = summary(fill_ms)
    moved = 4 * (b * t * (store.spf + 272) + b * t * 337) + (2 if store.audio_format == "int16" else 4) * b * t * store.spf + 4 * b * t * 272
    line["fill_bytes"] = moved
    line["fill_gb_per_s"] = round(moved / (np.median(fill_ms) * 1e-3) / 1e9, 1)

    # ---- the host path: gather_host into pinned memory, five copies, the reference's mask
    pinned = {k: torch.empty(v.shape, dtype=torch.float32).pin_memory() for k, v in loader.batch.items()}
    target = {k: torch.empty_like(v) for k, v in loader.batch.items()}
    order = data.epoch_order(store.n_clips, 0)
    n_host = max(1, args.fills // 10)

    def host_batch(i):
        ids = order[(i % len(loader)) * b:(i % len(loader) + 1) * b]
        store.gather_host(ids, out=pinned)
        for k in pinned:
            target[k].copy_(pinned[k], non_blocking=True)
        return (torch.rand(b, t, data.MASK_DIMS) < 0.3).float().to(dev)

    host_batch(0)
    torch.cuda.synchronize()
    host_ms = []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        for i in range(n_host):
            host_batch(i)
        torch.cuda.synchronize()
        host_ms.append(1e3 * (time.perf_counter() - t0) / n_host)
    line["host_path_ms"] = summary(host_ms)

    # ---- the captured step, static buffers vs the loader as prologue (two trainers on equal models, alternating runs)
    if not args.no_step:
        model_s, vq = workloads.product_models(precision=args.precision, device=dev)
        model_l, _ = workloads.product_models(precision=args.precision, device=dev)
        model_t, _ = workloads.product_models(precision=args.precision, device=dev)
        static = {k: v.to(dev) for k, v in workloads.train_batch(bs=b, t=t).items()}
        static["audio"] = static["audio"][:, :t * store.spf].contiguous()          # the loader's audio length (T * 533), so both arms run the same shapes
        static_mask = (torch.rand(b, t, data.MASK_DIMS, generator=torch.Generator().manual_seed(6)) < 0.5).float().to(dev)
        loader.set_epoch(0)
        loader.iteration = 0
        loader.mask_a, loader.mask_b = 0.0, 0.5                                    # the static arm's mask density
        ts = training.Trainer(model_s, vq, seed=1).capture(static, static_mask)
        tl = training.Trainer(model_l, vq, seed=1).capture(loader.batch, loader.random_mask, prologue=loader.fill)
        tt = training.Trainer(model_t, vq, seed=1).capture({k: v.clone() for k, v in static.items()}, static_mask.clone())
        for tr in (ts, tl, tt):
            tr.replay()
        torch.cuda.synchronize()
        ms = {"step_static_ms": [], "step_loader_ms": [], "step_static_twin_ms": []}
        losses = {}
        for _ in range(args.runs):
            for name, tr in (("step_static_ms", ts), ("step_loader_ms", tl), ("step_static_twin_ms", tt)):
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    losses[name] = tr.replay()
                torch.cuda.synchronize()
                ms[name].append(1e3 * (time.perf_counter() - t0) / args.steps)
        loader.check()
        for name, v in ms.items():
            line[name] = summary(v)
            assert all(np.isfinite(x) for x in losses[name].values()), (name, losses[name])
        line["step_loader_minus_static_ms"] = round(line["step_loader_ms"]["median"] - line["step_static_ms"]["median"], 4)
        line["clips_per_s_with_loader"] = round(b / (line["step_loader_ms"]["median"] * 1e-3), 1)
        line["step_twin_minus_static_ms"] = round(line["step_static_twin_ms"]["median"] - line["step_static_ms"]["median"], 4)
        line["loader_iteration"], line["skipped_steps"] = loader.iteration, [ts.skipped_steps, tl.skipped_steps, tt.skipped_steps]
        line["peak_memory_gb"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
