"""TEST-ONLY CPU stand-ins of the clip-store entry points (include/emage_hip.h: emage_gather_clips, emage_motion_mask), in the manner of
tests/fake_grad_clip.py: `installed()` is `fake_ops.installed()` plus `ops.gather_clips` and `ops.motion_mask` restated on host tensors, so
`data.ClipLoader` — order buffer, device counters, wrap of the cursor, status word — runs without a GPU.  Calls are recorded in
`fake_ops.CALLS` under the names in `NEW_CALLS`."""
import contextlib

import numpy as np
import torch

import fake_ops
from pantomatrix_amd import ops

NEW_CALLS = ("gather_clips", "motion_mask")


def gather_clips(order, cursor, n_batches, clips, arrays, out, status, *, frames, samples_per_frame):
    """emage_gather_clips as its header states it: batch position cursor mod n_batches, table rows {first frame, first sample, recording}, s16
    audio decoded x * 2^-15, an id outside the table (status 1) or a row outside the flat arrays (status 2) zero-fills its batch row."""
    fake_ops.CALLS.append("gather_clips")
    b = out["audio"].shape[0]
    assert order.dtype == torch.int32 and cursor.dtype == torch.int32 and status.dtype == torch.int32 and clips.dtype == torch.int64
    pos = int(cursor) % n_batches
    n_audio = frames * samples_per_frame
    for row in range(b):
        cid = int(order[pos * b + row])
        bad = 0
        if not 0 <= cid < clips.shape[0]:
            bad = 1
        else:
            f0, s0 = int(clips[cid, 0]), int(clips[cid, 1])
            if f0 < 0 or f0 + frames > arrays["motion"].shape[0] or s0 < 0 or s0 + n_audio > arrays["audio"].numel():
                bad = 2
        if bad:
            status |= bad
            for k in out:
                out[k][row] = 0
            continue
        for k in ops.CLIP_WIDTHS:
            out[k][row] = arrays[k][f0:f0 + frames]
        a = arrays["audio"][s0:s0 + n_audio]
        out["audio"][row] = a.to(torch.float32) * np.float32(1.0 / 32768.0) if a.dtype == torch.int16 else a
    return out


def motion_mask(out, a, b, seed, mask_id, iteration):
    fake_ops.CALLS.append("motion_mask")
    assert out.dtype == torch.float32 and iteration.dtype == torch.int32 and iteration.numel() == 1
    out.copy_(torch.from_numpy(ops.motion_mask_reference(out.numel(), a, b, int(seed), int(mask_id), int(iteration))).view(out.shape))
    return out


@contextlib.contextmanager
def installed():
    names = {"gather_clips": gather_clips, "motion_mask": motion_mask}
    with fake_ops.installed():
        saved = {n: getattr(ops, n) for n in names}
        try:
            for n, f in names.items():
                setattr(ops, n, f)
            yield
        finally:
            for n, f in saved.items():
                setattr(ops, n, f)
