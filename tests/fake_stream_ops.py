"""TEST-ONLY CPU stand-ins of the stream entry points (include/emage_hip.h: emage_stream_push, emage_stream_windows, emage_stream_commit,
emage_stream_emit), restated from the header's text in the manner of tests/fake_recording_ops.py: `installed()` is
`fake_recording_ops.installed()` plus the four ops on host tensors, so `streaming.StreamBatch` — rule 1's schedule, the rings, the segment
alignment, the carried translation, `close()` — runs without a GPU.  Calls are recorded in `fake_ops.CALLS` under the names in `NEW_CALLS`."""
import contextlib

import numpy as np
import torch

import fake_ops
import fake_recording_ops
from pantomatrix_amd import ops

NEW_CALLS = ("stream_push", "stream_windows", "stream_commit", "stream_emit")
READY, AUDIO_READ, AUDIO_WRITE, PUSH_COUNT, PUSH_SRC, CODE_WRITE, SEG_READ, SEG_VALID, EMIT_ROW, EMIT_COUNT = range(10)
BAD_PUSH, BAD_WINDOW, BAD_COMMIT, BAD_EMIT = 1, 2, 4, 8


def _table(table, slots):
    assert table.dtype == torch.int32 and tuple(table.shape) == (slots, ops.STREAM_WORDS)
    return table.tolist()


def stream_push(staged, table, ring, status):
    fake_ops.CALLS.append("stream_push")
    slots, ring_len = ring.shape
    for k, r in enumerate(_table(table, slots)):
        n, src, w = r[PUSH_COUNT], r[PUSH_SRC], r[AUDIO_WRITE]
        if n == 0:
            continue
        if n < 0 or n > ring_len or src < 0 or src + n > staged.numel() or w < 0 or w >= ring_len:
            status |= BAD_PUSH
            continue
        a = staged[src:src + n]
        a = a.to(torch.float32) * np.float32(1.0 / 32768.0) if a.dtype == torch.int16 else a
        ring[k, (w + torch.arange(n)) % ring_len] = a
    return ring


def stream_windows(ring, table, out, status):
    fake_ops.CALLS.append("stream_windows")
    slots, ring_len = ring.shape
    samples = out.shape[1]
    assert samples <= ring_len
    for k, r in enumerate(_table(table, slots)):
        out[k] = 0
        if not r[READY]:
            continue
        if r[AUDIO_READ] < 0 or r[AUDIO_READ] >= ring_len:
            status |= BAD_WINDOW
            continue
        out[k] = ring[k, (r[AUDIO_READ] + torch.arange(samples)) % ring_len]
    return out


def stream_commit(table, win_codes, keep, code_ring, segment, new_seed, seeds, status):
    fake_ops.CALLS.append("stream_commit")
    parts, slots, _window = win_codes.shape
    ring_codes, seg_len = code_ring.shape[2], segment.shape[2]
    for k, r in enumerate(_table(table, slots)):
        ok = bool(r[READY])
        if ok and not (0 <= r[CODE_WRITE] < ring_codes and 0 <= r[SEG_READ] < ring_codes and 0 <= r[SEG_VALID] <= min(seg_len, ring_codes)):
            status |= BAD_COMMIT
            ok = False
        segment[:, k] = 0
        if not ok:
            continue
        code_ring[:, k, (r[CODE_WRITE] + torch.arange(keep)) % ring_codes] = win_codes[:, k, :keep]
        seeds[k] = new_seed[k]
        segment[:, k, :r[SEG_VALID]] = code_ring[:, k, (r[SEG_READ] + torch.arange(r[SEG_VALID])) % ring_codes]
    return segment


def stream_emit(table, aa, expr, vel, col0, dt, segment, carry, poses, expressions, trans, codes, status):
    fake_ops.CALLS.append("stream_emit")
    parts, slots, seg_len = segment.shape
    out_rows = poses.shape[1]
    dt = np.float32(dt)
    for k, r in enumerate(_table(table, slots)):
        n, row = (r[EMIT_COUNT], r[EMIT_ROW]) if r[READY] else (0, 0)
        if r[READY] and (n < 0 or n > out_rows or row < 0 or row + n > seg_len):
            status |= BAD_EMIT
            n = 0
        for t in (poses, expressions, trans, codes):
            t[k] = 0
        if n == 0:
            continue
        lo = k * seg_len + row
        poses[k, :n], expressions[k, :n] = aa[lo:lo + n], expr[lo:lo + n]
        codes[k, :n] = segment[:, k, row:row + n].T
        v = vel[lo:lo + n, col0:col0 + 3].numpy()
        trans[k, :n, 1] = torch.from_numpy(v[:, 1].copy())
        for ax in (0, 2):
            pos = np.float32(carry[k, ax])
            for t in range(n):
                trans[k, t, ax] = float(pos)
                pos = np.float32(np.float32(v[t, ax] * dt) + pos)              # fadd(fmul(v, dt), pos), each rounded to fp32
            carry[k, ax] = float(pos)


@contextlib.contextmanager
def installed():
    names = {n: globals()[n] for n in NEW_CALLS}
    with fake_recording_ops.installed():
        saved = {n: getattr(ops, n) for n in names}
        try:
            for n, f in names.items():
                setattr(ops, n, f)
            yield
        finally:
            for n, f in saved.items():
                setattr(ops, n, f)
