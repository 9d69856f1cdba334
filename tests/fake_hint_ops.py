"""TEST-ONLY CPU stand-in of `ops.pack_motion_hints` (include/emage_hip.h: emage_pack_motion_hints) on top of
`fake_recording_ops.installed()`, so a `recordings.RecordingRunner(hints=True)` — hint store, table plan, `load()` — runs without a GPU.
The kernel is restated as its header states it: the dense (B, T, C) windows are materialised from the store by the table, rows outside the
store become rows without hints and set bit 2 of the status word, and the packing itself is `fake_ops.pack_motion`'s arithmetic.  Calls are
recorded in `fake_ops.CALLS` as "pack_motion_hints"."""
import contextlib

import torch

import fake_ops
import fake_recording_ops
from pantomatrix_amd import ops

NEW_CALLS = fake_recording_ops.NEW_CALLS + ("pack_motion_hints",)


def dense_windows(store_motion, store_keep, table, t, status=None):
    """-> motion (B, t, C) float32, mask (B, t, C) float32: what the table makes of the store.  Frames behind `avail` are masked (mask 1,
    motion 0: never used); a row outside the store is a row without hints and ORs 4 into `status`."""
    rows, c = store_motion.shape
    b = table.shape[0]
    motion, mask = torch.zeros(b, t, c), torch.ones(b, t, c)
    for k, (first, avail) in enumerate(table.tolist()):
        if avail < 0 or avail > t or first < 0 or first + avail > rows:
            if status is not None:
                status |= 4
            continue
        motion[k, :avail] = store_motion[first:first + avail]
        mask[k, :avail] = store_keep[first:first + avail].to(torch.float32)
    return motion, mask


def pack_motion_hints(dtype, store_motion, store_keep, table, emb, n_store, t, status, seed=None):
    assert store_motion.dtype == torch.float32 and store_keep.dtype == torch.uint8 and store_motion.shape == store_keep.shape
    assert store_motion.stride(1) == 1 and store_keep.stride(1) == 1 and store_motion.stride(0) == store_keep.stride(0) >= store_motion.shape[1]
    assert table.dtype == torch.int64 and table.dim() == 2 and table.shape[1] == 2 and table.is_contiguous() and status.dtype == torch.int32
    motion, mask = dense_windows(store_motion, store_keep, table, t, status)
    n = len(fake_ops.CALLS)
    out = fake_ops.pack_motion(dtype, motion, mask, emb, n_store, seed=seed)
    fake_ops.CALLS[n:] = ["pack_motion_hints"]
    return out


@contextlib.contextmanager
def installed():
    with fake_recording_ops.installed():
        saved = ops.pack_motion_hints
        try:
            ops.pack_motion_hints = pack_motion_hints
            yield
        finally:
            ops.pack_motion_hints = saved
