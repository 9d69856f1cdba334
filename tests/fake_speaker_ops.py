"""TEST-ONLY CPU stand-ins of the per-clip speaker entry points (include/emage_hip.h: emage_gather_clip_speakers,
emage_embedding_backward), in the manner of tests/fake_clip_ops.py: `installed()` is `fake_clip_ops.installed()` plus `ops.gather_clip_speakers`
and `ops.embedding_backward` restated on host tensors.  Calls are recorded in `fake_ops.CALLS` under the names in `NEW_CALLS`."""
import contextlib

import torch

import fake_clip_ops
import fake_ops
from pantomatrix_amd import ops

NEW_CALLS = ("gather_clip_speakers", "embedding_backward")


def gather_clip_speakers(order, cursor, n_batches, clips, speakers, out, status):
    """emage_gather_clip_speakers as its header states it: the batch position is cursor mod n_batches; an id outside the clip table writes 0
    and sets status bit 1, a recording id outside the speaker list (or a negative row) writes 0 and sets bit 2."""
    fake_ops.CALLS.append("gather_clip_speakers")
    assert order.dtype == torch.int32 and cursor.dtype == torch.int32 and status.dtype == torch.int32
    assert clips.dtype == torch.int64 and speakers.dtype == torch.int64 and out.dtype == torch.int64 and out.is_contiguous()
    b = out.numel()
    pos = int(cursor) % n_batches
    flat = out.view(-1)
    for row in range(b):
        cid = int(order[pos * b + row])
        if not 0 <= cid < clips.shape[0]:
            status |= 1
            flat[row] = 0
            continue
        r = int(clips[cid, 2])
        if not 0 <= r < speakers.numel() or int(speakers[r]) < 0:
            status |= 2
            flat[row] = 0
            continue
        flat[row] = int(speakers[r])
    return out


def embedding_backward(g, ids, rows, dw=None):
    """emage_embedding_backward: per-clip float64 sums over T, then per table row the sums of its clips in ascending clip order; ids clamped
    as the forward gather clamps; rows no clip names are zero; the result is written, not accumulated."""
    fake_ops.CALLS.append("embedding_backward")
    ids = ids.reshape(-1).clamp(0, rows - 1)
    b, d = ids.numel(), g.shape[1]
    per_clip = g.double().reshape(b, -1, d).sum(1)
    acc = torch.zeros(rows, d, dtype=torch.float64)
    acc.index_add_(0, ids, per_clip)
    res = acc.to(torch.float32)
    if dw is None:
        return res
    dw.copy_(res)
    return dw


@contextlib.contextmanager
def installed():
    names = {"gather_clip_speakers": gather_clip_speakers, "embedding_backward": embedding_backward}
    with fake_clip_ops.installed():
        saved = {n: getattr(ops, n) for n in names}
        try:
            for n, f in names.items():
                setattr(ops, n, f)
            yield
        finally:
            for n, f in saved.items():
                setattr(ops, n, f)
