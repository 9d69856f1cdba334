"""TEST-ONLY CPU stand-in of emage_stream_push_resample (include/emage_hip.h), restated from the header's text beside tests/fake_stream_ops.py:
the decode, the channel mean and the polyphase sum in fp32 in the kernel's order — taps of a phase row in row order, each step one fused
multiply-add (the product of two fp32 values is exact in float64 and the sum is rounded to fp32 from there).  `installed()` is
`fake_stream_ops.installed()` plus this op, so a `StreamBatch(audio_inputs=...)` runs without a GPU; `resample_whole` is the same
arithmetic over a whole recording, the stand-in of `ops.audio_resample` the streamed samples are compared with."""
import contextlib

import numpy as np
import torch

import fake_ops
import fake_stream_ops
from pantomatrix_amd import audio, ops

NEW_CALLS = ("stream_push_resample",)
FRAMES, SRC16, FORMAT, FINAL, OUT_COUNT, OUT_POS, KMAX0, R0, HIST_VALID, HIST_SIDE = range(10)
BAD_RESAMPLE = 16
_F32 = np.float32


def decode(raw, pcm, channels):
    """raw: uint8 bytes of whole interleaved frames -> (n,) float32 mono: the sample decode and the fp32 channel mean of csrc/pcm_taps.h."""
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    if pcm == 0:
        x = raw.view("<i2").astype(_F32) * _F32(1.0 / 32768.0)
    elif pcm == 1:
        b = raw.reshape(-1, 3).astype(np.int64)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        x = ((v ^ 0x800000) - 0x800000).astype(_F32) * _F32(1.0 / 8388608.0)
    elif pcm == 2:
        x = raw.view("<i4").astype(_F32) * _F32(1.0 / 2147483648.0)
    else:
        x = raw.view("<f4").copy()
    x = x.reshape(-1, channels)
    s = x[:, 0].copy()
    for c in range(1, channels):
        s = (s + x[:, c]).astype(_F32)
    return s if channels == 1 else (s / _F32(channels)).astype(_F32)


def _walk(ext, off, kmax, phase, fmt, taps):
    """Outputs whose newest frame is kmax[j] and phase row phase[j]; frame k of the session lives at ext[k + off]."""
    _pcm, _ch, up, down, _half, rpp, pitch, t0 = fmt
    if up == down:
        return ext[kmax + off].astype(_F32)
    acc = np.zeros(len(kmax), dtype=_F32)
    for i in range(rpp):
        h = taps[t0 + phase * pitch + i].astype(np.float64)
        acc = (h * ext[kmax - i + off].astype(np.float64) + acc.astype(np.float64)).astype(_F32)
    return acc


def resample_whole(raw, audio_input):
    """A whole recording's bytes -> the float32 samples `ops.audio_resample` stands for, in this module's arithmetic."""
    desc, taps, _h = ops.stream_formats((audio_input,))
    fmt = [int(v) for v in desc[0]]
    _pcm, ch, up, down, half, rpp = fmt[:6]
    x = decode(raw, fmt[0], ch)
    m = np.arange(audio.out_length(len(x), up, down), dtype=np.int64)
    kmax = (m * down + half) // up
    ext = np.concatenate([np.zeros(rpp, _F32), x, np.zeros(int(kmax.max(initial=0)) + 1, _F32)])
    return _walk(ext, rpp, kmax, (m * down + half) % up, fmt, taps)


def stream_push_resample(staged, rs_table, formats, taps, ring, history, status):
    fake_ops.CALLS.append("stream_push_resample")
    slots, ring_len = ring.shape
    hist_len = history.shape[2]
    formats = np.asarray(formats).reshape(-1, ops.STREAM_FORMAT_WORDS)
    assert rs_table.dtype == torch.int32 and tuple(rs_table.shape) == (slots, ops.STREAM_RS_WORDS) and staged.dtype == torch.uint8
    taps, raw = taps.numpy(), staged.numpy()
    for k, r in enumerate(rs_table.tolist()):
        n, count = r[FRAMES], r[OUT_COUNT]
        if n == 0 and count == 0:
            continue
        ok = (0 <= r[FORMAT] < len(formats) and n >= 0 and r[SRC16] >= 0 and 0 <= count <= ring_len and 0 <= r[OUT_POS] < ring_len and r[KMAX0] >= 0
              and r[R0] >= 0 and 0 <= r[HIST_VALID] <= hist_len and r[HIST_SIDE] in (0, 1))
        if ok:
            fmt = [int(v) for v in formats[r[FORMAT]]]
            pcm, ch, up, down = fmt[:4]
            fb = ch * (2, 3, 4, 4)[pcm]
            j = np.arange(count, dtype=np.int64)
            kmax, phase = r[KMAX0] + (j * down + r[R0]) // up, (j * down + r[R0]) % up
            ok = r[R0] < up and r[SRC16] * 16 + n * fb <= len(raw) and (r[FINAL] or count == 0 or int(kmax[-1]) < n)
        if not ok:
            status |= BAD_RESAMPLE
            continue
        old = history[k, r[HIST_SIDE]].numpy().copy()
        old[:hist_len - r[HIST_VALID]] = 0                                         # frames before the session's start
        behind = max(int(kmax[-1]) - n + 1, 0) if count else 0                     # zeros behind the end: read only under FINAL
        ext = np.concatenate([old, decode(raw[r[SRC16] * 16:r[SRC16] * 16 + n * fb], pcm, ch), np.zeros(behind, _F32)])
        if count:
            ring[k, (r[OUT_POS] + torch.arange(count)) % ring_len] = torch.from_numpy(_walk(ext, hist_len, kmax, phase, fmt, taps))
        if n:
            history[k, 1 - r[HIST_SIDE]] = torch.from_numpy(ext[n:n + hist_len].copy())
    return ring


@contextlib.contextmanager
def installed():
    with fake_stream_ops.installed():
        saved = ops.stream_push_resample
        ops.stream_push_resample = stream_push_resample
        try:
            yield
        finally:
            ops.stream_push_resample = saved
