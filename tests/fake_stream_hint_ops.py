"""TEST-ONLY CPU stand-in of `ops.stream_push_hints` (include/emage_hip.h: emage_stream_push_hints), restated from the header's text in the
manner of tests/fake_stream_ops.py: `installed()` is `fake_stream_ops.installed()` and `fake_hint_ops.installed()` plus this op on host
tensors, so a `streaming.StreamBatch(motion_hints=True)` — rule 5's gating, the hint rings and their mirror rows, the window table, the seed
rows, `close()` — runs without a GPU.  `ring_model` is the same arithmetic on numpy arrays, for the kernel tests.  Calls are recorded in
`fake_ops.CALLS` as "stream_push_hints"."""
import contextlib

import numpy as np
import torch

import fake_hint_ops
import fake_ops
import fake_stream_ops
from pantomatrix_amd import ops, recordings

NEW_CALLS = ("stream_push_hints",)
COUNT, SRC16, FORM, WRITE, SEED_ROW, SEED_COUNT, READY, WIN_FIRST, WIN_AVAIL = range(9)
BAD_HINTS = 32
C, PRE = 337, 4


def stage(chunks, staged_bytes=None):
    """[(form, motion (n, W) float32, mask (n, 337) uint8)] -> (the staged bytes as the header lays them out, every chunk from a 16-byte
    boundary; [byte offset of each chunk])."""
    offsets, lo = [], 0
    for form, motion, _mask in chunks:
        offsets.append(lo)
        lo += ops.stream_hint_chunk_bytes(len(motion), form)
    buf = np.zeros(max(lo, 16) if staged_bytes is None else staged_bytes, dtype=np.uint8)
    for (form, motion, mask), at in zip(chunks, offsets):
        n, w = motion.shape
        assert w == ops.STREAM_HINT_WIDTHS[form] and mask.shape == (n, C)
        buf[at:at + n * w * 4] = np.ascontiguousarray(motion, dtype=np.float32).view(np.uint8).reshape(-1)
        buf[at + n * w * 4:at + n * (w * 4 + C)] = np.ascontiguousarray(mask, dtype=np.uint8).reshape(-1)
    return buf, offsets


def _row_ok(r, staged_bytes, hint_rows, window):
    w = ops.STREAM_HINT_WIDTHS[r[FORM]] if r[FORM] in (0, 1) else 0
    ok = 0 <= r[COUNT] <= hint_rows and r[SRC16] >= 0 and r[FORM] in (0, 1) and 0 <= r[WRITE] < hint_rows
    ok = ok and r[SRC16] * 16 + r[COUNT] * (w * 4 + C) <= staged_bytes
    if ok and r[SEED_COUNT] != 0:
        ok = r[SEED_COUNT] > 0 and r[SEED_ROW] == r[WRITE] and r[SEED_ROW] + r[SEED_COUNT] <= PRE and r[SEED_COUNT] <= r[COUNT]
    if ok and r[READY]:
        ok = 0 <= r[WIN_AVAIL] <= window and r[WIN_FIRST] >= 0 and r[WIN_FIRST] + window <= hint_rows + PRE
    return ok


def ring_model(staged, table, ring_motion, ring_keep, seeds, window_table, window, rot6d=None):
    """The header's text on numpy arrays, in place -> the status bits.  rot6d: (n, 55, 3) float32 -> (n, 55, 6), the conversion of the
    tracker form (None: `recordings.axis_angle_to_rot6d`, the host arithmetic)."""
    slots, rows, _ld = ring_motion.shape
    hint_rows, status = rows - PRE, 0
    if rot6d is None:
        rot6d = lambda aa: recordings.axis_angle_to_rot6d(torch.from_numpy(aa)).numpy()
    for k, r in enumerate(np.asarray(table).tolist()):
        window_table[k] = 0
        if not _row_ok(r, staged.size, hint_rows, window):
            status |= BAD_HINTS
            continue
        if r[READY]:
            window_table[k] = [k * rows + r[WIN_FIRST], r[WIN_AVAIL]]
        n = r[COUNT]
        if n == 0:
            continue
        w, lo = ops.STREAM_HINT_WIDTHS[r[FORM]], r[SRC16] * 16
        data = staged[lo:lo + n * w * 4].view(np.float32).reshape(n, w)
        mask = staged[lo + n * w * 4:lo + n * (w * 4 + C)].reshape(n, C)
        motion = data
        if r[FORM] == ops.STREAM_HINT_TRACKER:
            motion = np.concatenate([rot6d(np.ascontiguousarray(data[:, :165]).reshape(n, 55, 3)).reshape(n, 330), data[:, 165:]], axis=1)
        for j in range(n):
            p = (r[WRITE] + j) % hint_rows
            for q in [p] + ([hint_rows + p] if p < PRE else []):
                ring_motion[k, q, :C], ring_motion[k, q, C:] = motion[j], 0.0
                ring_keep[k, q, :C], ring_keep[k, q, C:] = mask[j], 1
            if j < r[SEED_COUNT]:
                seeds[k, r[SEED_ROW] + j] = motion[j]
    return status


def stream_push_hints(staged, hint_table, ring_motion, ring_keep, seeds, window_table, window, status):
    fake_ops.CALLS.append("stream_push_hints")
    slots = ring_motion.shape[0]
    assert hint_table.dtype == torch.int32 and tuple(hint_table.shape) == (slots, ops.STREAM_HINT_WORDS)
    assert staged.dtype == torch.uint8 and window_table.dtype == torch.int64 and tuple(window_table.shape) == (slots, 2)
    assert ring_motion.is_contiguous() and ring_keep.is_contiguous() and seeds.is_contiguous() and tuple(seeds.shape) == (slots, PRE, C)
    bits = ring_model(staged.numpy(), hint_table.numpy(), ring_motion.numpy(), ring_keep.numpy(), seeds.numpy(), window_table.numpy(), int(window))
    if bits:
        status |= bits
    return window_table


@contextlib.contextmanager
def installed():
    with fake_hint_ops.installed(), fake_stream_ops.installed():
        saved = ops.stream_push_hints
        try:
            ops.stream_push_hints = stream_push_hints
            yield
        finally:
            ops.stream_push_hints = saved
