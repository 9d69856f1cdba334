"""TEST-ONLY CPU stand-ins of the recording-pass entry points (include/emage_hip.h: emage_gather_windows, emage_copy_segments), in the manner
of tests/fake_clip_ops.py: `installed()` is `fake_ops.installed()` plus `ops.gather_windows` and `ops.copy_segments` restated on host tensors,
so `recordings.RecordingRunner` — schedule, seed chain, tail groups, per-length decode, packing in input order — runs without a GPU.
Calls are recorded in `fake_ops.CALLS` under the names in `NEW_CALLS`."""
import contextlib

import numpy as np
import torch

import fake_ops
from pantomatrix_amd import ops

NEW_CALLS = ("gather_windows", "copy_segments")


def gather_windows(audio, offsets, out, status):
    """emage_gather_windows as its header states it: row b = audio[offsets[b] : + samples], s16 decoded x * 2^-15; a window outside the
    array is zero-filled and sets bit 0 of the status word."""
    fake_ops.CALLS.append("gather_windows")
    assert offsets.dtype == torch.int64 and status.dtype == torch.int32 and out.dtype == torch.float32 and offsets.numel() == out.shape[0]
    samples = out.shape[1]
    for b in range(out.shape[0]):
        s0 = int(offsets[b])
        if s0 < 0 or s0 + samples > audio.numel():
            status |= 1
            out[b] = 0
            continue
        a = audio[s0:s0 + samples]
        out[b] = a.to(torch.float32) * np.float32(1.0 / 32768.0) if a.dtype == torch.int16 else a
    return out


def copy_segments(src, dst, segments, width_bytes, max_rows, status):
    """emage_copy_segments: rows of `width_bytes` bytes, {first source row, first destination row, rows}; a segment outside its buffers or
    longer than max_rows is skipped and sets bit 1 of the status word."""
    fake_ops.CALLS.append("copy_segments")
    assert src.is_contiguous() and dst.is_contiguous() and src.dtype == dst.dtype and segments.dtype == torch.int64 and status.dtype == torch.int32
    s = src.view(-1).view(torch.uint8).view(-1, width_bytes)
    d = dst.view(-1).view(torch.uint8).view(-1, width_bytes)
    for sr, dr, n in segments.tolist():
        if n < 0 or n > max_rows or sr < 0 or sr + n > s.shape[0] or dr < 0 or dr + n > d.shape[0]:
            status |= 2
            continue
        d[dr:dr + n] = s[sr:sr + n]
    return dst


@contextlib.contextmanager
def installed():
    names = {"gather_windows": gather_windows, "copy_segments": copy_segments}
    with fake_ops.installed():
        saved = {n: getattr(ops, n) for n in names}
        try:
            for n, f in names.items():
                setattr(ops, n, f)
            yield
        finally:
            for n, f in saved.items():
                setattr(ops, n, f)
