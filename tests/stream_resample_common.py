"""Shared by the streaming-resampler tests (host and GPU): PCM in every push layout, a harness that drives `ops.stream_push_resample` (or
its stand-in) over several slots with the host's bookkeeping written out independently of `streaming.py`, chunking plans, and a driver
that runs sessions of a `StreamBatch` which open and close at different ticks."""
import numpy as np
import torch

import audio_common
import stream_common as sc
from pantomatrix_amd import _lib, audio, ops

TILE = _lib.AUDIO_TILE
CANARY = -7.0
PAD = 64                                                 # canary elements either side of a buffer (a multiple of 16 bytes for every dtype)


def hi_frames(rate):
    """The fewest frames with n_out >= 2 TILE + 1: three output tiles, the last one short (`tile_frame_counts(rate)[0]` of
    test_audio_frontend_gpu.py)."""
    up, down = audio.rate_ratio(rate, 16000)
    hi = (2 * TILE) * down // up + 1
    assert audio.out_length(hi, up, down) >= 2 * TILE + 1 > audio.out_length(hi - 1, up, down)
    return hi


def encode(x16, fmt):
    """(n, ch) int16 -> the frames as `Session.push` takes them in format `fmt`: the same sample values scaled to the format's width (s24 / s32:
    shifted up, the low bits filled from the sample itself), as test_audio_frontend_gpu.encode lays them out."""
    x = x16.astype(np.int64)
    n, ch = x.shape
    if fmt == "s16":
        return np.ascontiguousarray(x16)
    if fmt == "s24":
        u = ((x << 8) | (x & 0xFF)) & 0xFFFFFF
        return np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=-1).astype(np.uint8).reshape(n, ch * 3)
    if fmt == "s32":
        return ((x << 16) | (x & 0xFFFF)).astype(np.int32)
    return ((x16.astype(np.float32) / 32768.0) * np.float32(1.0001)).astype(np.float32)


def exact_mono(pcm, inp):
    """The float64 mono signal the bytes of `pcm` (push layout) stand for, exact where the channel mean is (s16 / f32 of up to 2 channels)."""
    if inp.fmt == "s16":
        return pcm.astype(np.float64).mean(axis=1) / 32768.0
    assert inp.fmt == "f32"
    return pcm.astype(np.float64).mean(axis=1)


def clip(inp, n, seed, which=0):
    """Seeded frames of `inp`'s layout: clip `which` of audio_common.pcm_clips (2: full-scale alternating)."""
    return encode(audio_common.pcm_clips(n, inp.channels, seed)[which], inp.fmt)


def as_bytes(pcm):
    return np.ascontiguousarray(pcm).view(np.uint8).reshape(-1)


def plans(n, rpp, up, down):
    """The four ways a recording of n frames is cut: {name: [chunk lengths]}."""
    def cut(sizes, rest):
        out, left = [], n
        for c in sizes:
            if left <= 0:
                break
            out.append(min(c, left))
            left -= out[-1]
        while left > 0:
            out.append(min(rest, left))
            left -= out[-1]
        return out
    tile_frames = max(TILE * down // up, 1)              # about one output tile's worth of input
    return {"frame by frame, then 997": cut([1] * (3 * rpp), 997), "shorter than rpp": cut([], max(rpp - 1, 1)), "one chunk": [n],
            "one output tile": cut([], tile_frames)}


def ring_for(plans_, up, down):
    """The smallest comfortable ring for these chunkings: the outputs of the largest chunk (or of the flush, at most 21) and 13 more.  A
    chunked feed then wraps inside its chunks again and again; a recording pushed as ONE chunk needs a ring that holds all of its outputs."""
    return max(max(-(-max(p) * up // down) + 2 for p in plans_), 22) + 13


def buffer(shape, dtype, dev, fill=CANARY):
    """A contiguous tensor of `shape` with PAD canary elements either side -> (whole 1-D buffer, the view)."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=dev)
    return whole, whole[PAD:PAD + n].view(*shape)


def canaries_intact(whole, fill=CANARY):
    return bool((whole[:PAD] == fill).all()) and bool((whole[-PAD:] == fill).all())


class Harness:
    """`slots` slots of the op under test, each with its own format and the host's counters (frames sent, outputs written, history side),
    kept here in plain Python integers.  `launch({slot: (frames in push layout, final)})` stages, builds the table, calls `op`, un-wraps the
    ring and checks that exactly the outputs that became final were written and nothing else in the ring moved."""

    def __init__(self, inputs, slot_formats, ring_len, dev, op=None, staged_bytes=1 << 20):
        self.inputs, self.dev, self.op = tuple(inputs), dev, op or ops.stream_push_resample
        self.desc, taps, self.hist_len = ops.stream_formats(self.inputs)
        self.slot_formats, self.slots, self.ring_len = list(slot_formats), len(slot_formats), ring_len
        self.taps_whole, self.taps = buffer((len(taps),), torch.float32, dev)
        self.taps.copy_(torch.from_numpy(taps))
        self.ring_whole, self.ring = buffer((self.slots, ring_len), torch.float32, dev)
        self.hist_whole, self.history = buffer((self.slots, 2, self.hist_len), torch.float32, dev)
        self.staged_whole, self.staged = buffer((staged_bytes,), torch.uint8, dev, fill=0xA5)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.sent, self.written, self.side = [0] * self.slots, [0] * self.slots, [0] * self.slots
        self.out = [[] for _ in range(self.slots)]
        self.snapshot = self.ring.cpu().clone()

    def ratio(self, k):
        return audio.rate_ratio(self.inputs[self.slot_formats[k]].rate, 16000)

    def reopen(self, k, fmt):
        """A new session in slot k: the counters start over, the device buffers keep what they hold."""
        self.slot_formats[k], self.sent[k], self.written[k], self.out[k] = fmt, 0, 0, []

    def rows(self, pushes):
        rows, lo, host = [None] * self.slots, 0, np.zeros(self.staged.numel(), dtype=np.uint8)
        for k, (pcm, final) in sorted(pushes.items()):
            up, down = self.ratio(k)
            raw, frames = as_bytes(pcm), len(pcm)
            total = self.sent[k] + frames
            upto = audio.out_length(total, up, down) if final else audio.available(total, up, down)
            host[lo:lo + len(raw)] = raw
            rows[k] = dict(frames=frames, src=lo, format=self.slot_formats[k], final=int(final), frames_before=self.sent[k],
                           outputs_before=self.written[k], out_count=upto - self.written[k], hist_side=self.side[k])
            lo += -(-len(raw) // 16) * 16
        return rows, host, lo

    def launch(self, pushes):
        rows, host, used = self.rows(pushes)
        tab = ops.stream_resample_table(rows, formats=self.desc, ring_len=self.ring_len, staged_bytes=self.staged.numel(), hist_len=self.hist_len)
        if used:
            self.staged[:used].copy_(torch.from_numpy(host[:used]))
        self.op(self.staged, torch.from_numpy(tab).to(self.dev), self.desc, self.taps, self.ring, self.history, self.status)
        ring = self.ring.cpu()
        moved = torch.zeros_like(ring, dtype=torch.bool)
        for k, row in enumerate(rows):
            if row is None:
                continue
            pos = (row["outputs_before"] + torch.arange(row["out_count"])) % self.ring_len
            self.out[k].append(ring[k, pos].numpy().copy())
            moved[k, pos] = True
            self.sent[k] += row["frames"]
            self.written[k] += row["out_count"]
            if row["frames"]:
                self.side[k] ^= 1
        assert torch.equal(ring[~moved], self.snapshot[~moved]), "a ring position outside the outputs that became final was written"
        assert not torch.isnan(ring[moved]).any() and int(self.status) == 0
        self.snapshot = ring.clone()

    def result(self, k):
        return np.concatenate(self.out[k]) if self.out[k] else np.zeros(0, np.float32)


def run_plan(h, pcm_by_slot, plan_by_slot):
    """Feeds every slot its recording in its own chunking, one chunk of each slot per launch, then flushes each with the final flag in a
    launch of its own kind: the last chunk of the longest plan travels with the flags of the slots that ended earlier."""
    pos = {k: 0 for k in pcm_by_slot}
    todo = {k: list(p) for k, p in plan_by_slot.items()}
    ended = set()
    while len(ended) < len(pcm_by_slot):
        pushes = {}
        for k, pcm in pcm_by_slot.items():
            if k in ended:
                continue
            if todo[k]:
                c = todo[k].pop(0)
                pushes[k] = (pcm[pos[k]:pos[k] + c], False)
                pos[k] += c
            else:
                pushes[k] = (pcm[:0], True)                # no frames, the final flag: a flush
                ended.add(k)
        h.launch(pushes)
        for k in pushes:
            up, down = h.ratio(k)
            want = audio.out_length(pos[k], up, down) if k in ended else audio.available(pos[k], up, down)
            assert h.written[k] == want and h.sent[k] == pos[k]


# ---- sessions of a StreamBatch ---------------------------------------------------------------------------------------------------------------
def run_sessions(sb, plan):
    """plan: [(tick the session opens at, its audio — frames of its format, or 16 kHz float samples —, AudioInput or None, chunk length)].
    Every tick each live session is fed chunk by chunk until its next window is ready or its audio is used up (then `end()`), the batch steps,
    and sessions that are used up and not ready close -> ([joined output per session], [slot per session])."""
    n = len(plan)
    sess, pos, acc, slots, done = [None] * n, [0] * n, [[] for _ in range(n)], [None] * n, [False] * n
    tick = 0
    while not all(done):
        for i, (t0, _pcm, inp, _c) in enumerate(plan):
            if t0 == tick:
                sess[i] = sb.open(audio_input=inp) if inp is not None else sb.open()
                slots[i] = sess[i].slot
        live = [i for i in range(n) if sess[i] is not None and not done[i]]
        for i in live:
            pcm, c = plan[i][1], plan[i][3]
            while not sess[i].ready and pos[i] < len(pcm):
                sess[i].push(pcm[pos[i]:pos[i] + c])
                pos[i] = min(pos[i] + c, len(pcm))
            if pos[i] >= len(pcm):
                sess[i].end()
        out = sb.step()
        for i in live:
            if sess[i] in out:
                acc[i].append(out[sess[i]])
            elif pos[i] >= len(plan[i][1]):
                acc[i].append(sess[i].close())
                done[i] = True
        tick += 1
        assert tick < 64
    return [sc.joined(a) for a in acc], slots


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and all(np.array_equal(a[3][p], b[3][p]) for p in a[3])
