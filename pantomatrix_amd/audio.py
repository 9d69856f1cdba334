"""The audio front end on the device: WAV file -> mono float32 at the model's 16 kHz, the `librosa.load(path, sr=16000)` of
test_emage_audio.py:17-18 for PCM input, as ONE launch (`emage_audio_resample`: decode, channel mean, polyphase low-pass resampling).

Host side of it, numpy only:
* ``resample_filter(up, down)``   the float64 taps `scipy.signal.resample_poly(x, up, down)` designs by default;
* ``resample_host(x, up, down)``  the float64 polyphase sum the kernel restates in fp32 — the ORACLE of the GPU tests, not a fallback;
* ``pack_taps / unpack_taps``     the phase-row layout the kernel keeps in LDS; ``packed_taps`` caches it per (up, down, device).
``load_audio(path, sr, device)`` uploads a file's raw PCM and resamples it there; ``AudioInput`` describes the PCM a ``ClipRunner``
takes in place of 16 kHz float audio."""
from __future__ import annotations

from dataclasses import dataclass
from math import gcd

import numpy as np

from . import motion_io
from ._lib import PCM_S16, PCM_S24, PCM_S32, PCM_F32

PCM_FORMATS = {"s16": PCM_S16, "s24": PCM_S24, "s32": PCM_S32, "f32": PCM_F32}
_TAPS = {}        # (up, down, device) -> packed float32 phase rows on that device


def rate_ratio(in_rate, out_rate):
    """(up, down) in lowest terms: out_rate / in_rate."""
    g = gcd(int(in_rate), int(out_rate))
    return int(out_rate) // g, int(in_rate) // g


def half_length(up, down):
    return 10 * max(up, down)


def out_length(n_in, up, down):
    """ceil(n_in * up / down): the output frames of `n_in` input frames."""
    return -(-int(n_in) * up // down)


def stream_half(up, down):
    """The filter's reach as a STREAM sees it: `half_length`, and 0 where up == down (the kernels only decode there: no filter, nothing held back)."""
    return 0 if up == down else half_length(up, down)


def available(n_in, up, down):
    """Outputs that are FINAL after `n_in` input frames: output m reads frames up to kmax = (m down + half) // up, so it no longer depends on
    what follows once n_in > kmax, i.e. m down + half < n_in up — the first ceil((n_in up - half) / down) outputs (the streaming
    front end).  Never more than `out_length(n_in, up, down)`; the outputs between the two wait for more input or for the end of the stream."""
    return max(0, -(-(int(n_in) * up - stream_half(up, down)) // down))


def resample_filter(up, down):
    """The float64 taps of `scipy.signal.resample_poly(x, up, down)`'s default filter: 2 * half + 1 taps of a windowed-sinc low-pass with
    cutoff 1 / max(up, down) of Nyquist, Kaiser window beta = 5, unit gain at DC, times `up`."""
    half = half_length(up, down)
    cutoff = 1.0 / max(up, down)
    m = np.arange(-half, half + 1, dtype=np.float64)
    h = cutoff * np.sinc(cutoff * m) * np.kaiser(2 * half + 1, 5.0)
    return h / h.sum() * up


def _tap_walk(m, n, up, down):
    """For outputs `m` (int64 array): tap indices j (len(m), rpp), input indices k, and which of them exist
    (0 <= j <= 2 half, 0 <= k < n).  Output m reads h[j] * x[k] with j = (m down + half) mod up + i up and k = (m down + half) // up - i."""
    half = half_length(up, down)
    rpp = -(-(2 * half + 1) // up)
    base = m.astype(np.int64) * down + half
    i = np.arange(rpp, dtype=np.int64)
    j = (base % up)[:, None] + i[None, :] * up
    k = (base // up)[:, None] - i[None, :]
    return j, k, (j <= 2 * half) & (k >= 0) & (k < n)


def resample_host(x, up, down, h=None, chunk=1 << 14):
    """y[m] = sum_k h[m down + half - k up] x[k] in float64, n_out = ceil(n up / down) outputs: `scipy.signal.resample_poly(x, up, down)`
    written as the polyphase sum the kernel computes.  `h`: other taps of the same length (the tests pass the fp32-rounded ones)."""
    x = np.asarray(x, dtype=np.float64)
    h = resample_filter(up, down) if h is None else np.asarray(h, dtype=np.float64)
    n = x.shape[0]
    y = np.empty(out_length(n, up, down), dtype=np.float64)
    for m0 in range(0, len(y), chunk):
        m = np.arange(m0, min(m0 + chunk, len(y)))
        j, k, ok = _tap_walk(m, n, up, down)
        y[m] = np.where(ok, h[np.where(ok, j, 0)] * x[np.where(ok, k, 0)], 0.0).sum(axis=1)
    return y


def phase_pitch(n_taps, up):
    """Floats per phase row: the taps of the longest phase, made odd (lane l reads row (r0 + l down) mod up; with an odd pitch rows that differ
    mod 32 start on different banks of the 32 a one-float LDS read is served from — csrc/audio.hip has the whole pattern)."""
    return -(-n_taps // up) | 1


def pack_taps(h, up):
    """(n_taps,) -> (up, phase_pitch) float32: row p = h[p], h[p + up], h[p + 2 up], ..., then zeros."""
    h = np.asarray(h)
    rows = np.zeros((up, phase_pitch(len(h), up)), dtype=np.float32)
    for p in range(up):
        t = h[p::up]
        rows[p, :len(t)] = t
    return rows


def unpack_taps(rows, n_taps):
    """Inverse of `pack_taps`: the (n_taps,) taps of an (up, pitch) table."""
    rows = np.asarray(rows)
    up = rows.shape[0]
    h = np.empty(n_taps, dtype=rows.dtype)
    for p in range(up):
        t = h[p::up]
        t[:] = rows[p, :len(t)]
    return h


def packed_taps(up, down, device):
    """The phase rows of `resample_filter(up, down)` as a float32 tensor on `device`, built once per (up, down, device).  The first call for a
    key designs the filter on the host and uploads it: make it BEFORE a stream capture that records `ops.audio_resample` for that rate pair
    (`ClipRunner` does, in its constructor)."""
    import torch
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (up, down, str(device))
    if key not in _TAPS:
        _TAPS[key] = torch.from_numpy(pack_taps(resample_filter(up, down), up)).to(device)
    return _TAPS[key]


@dataclass(frozen=True)
class AudioInput:
    """The PCM a `ClipRunner(audio_input=...)` is fed in place of 16 kHz float audio: sample rate, channels and sample format
    ("s16", "s24" = packed 3-byte little endian, "s32", "f32")."""
    rate: int
    channels: int
    fmt: str = "s16"

    def __post_init__(self):
        if self.fmt not in PCM_FORMATS:
            raise ValueError(f"AudioInput.fmt must be one of {sorted(PCM_FORMATS)}, not {self.fmt!r}")

    def frames_for(self, n_samples, out_rate=16000):
        """The smallest frame count whose resampled length reaches `n_samples`."""
        up, down = rate_ratio(self.rate, out_rate)
        return (int(n_samples) - 1) * down // up + 1          # ceil(n up / down) >= n_samples  <=>  n up > (n_samples - 1) down

    def staging(self, batch, n_in, device):
        """A zeroed (batch, n_in, ...) tensor of this format, as `ops.audio_resample` takes it."""
        import torch
        dtype = {"s16": torch.int16, "s24": torch.uint8, "s32": torch.int32, "f32": torch.float32}[self.fmt]
        return torch.zeros(batch, n_in, self.channels * (3 if self.fmt == "s24" else 1), dtype=dtype, device=device)


def _pcm_tensor(path):
    """A WAV file's samples as `ops.audio_resample` takes them, still on the host: ((1, n, ch [* 3]) tensor, channels, sample rate).  16 / 24 / 32-bit
    PCM and float32 keep the `data` chunk's bytes as they are; 8-bit and float64 files are decoded here and passed on as float32."""
    import torch
    (tag, ch, sr, _, _, bits), data = motion_io._wav_chunks(path)
    if (tag, bits) in ((1, 16), (1, 24), (1, 32), (3, 32)):
        fb = ch * bits // 8
        n = len(data) // fb
        raw = np.frombuffer(data, dtype=np.uint8, count=n * fb)
        if bits != 24:
            raw = raw.view({(1, 16): "<i2", (1, 32): "<i4", (3, 32): "<f4"}[(tag, bits)])
        return torch.from_numpy(raw.reshape(1, n, -1).copy()), ch, sr
    x, sr = motion_io._read_wav(path)
    return torch.from_numpy(np.ascontiguousarray(x))[None], ch, sr


def load_audio(path, sr=16000, device=None):
    """`motion_io.load_audio` with the work on the device.  device=None: exactly `motion_io.load_audio(path, sr)` (host, numpy array).
    With a device: the RIFF header is parsed here, the file's PCM is uploaded as it is, and one `emage_audio_resample` launch decodes,
    down-mixes and resamples it -> (audio (n_out,) float32 tensor on the device, sr)."""
    if device is None:
        return motion_io.load_audio(path, sr)
    from . import ops
    pcm, ch, in_sr = _pcm_tensor(path)
    return ops.audio_resample(pcm.to(device), ch, in_sr, sr)[0], sr
