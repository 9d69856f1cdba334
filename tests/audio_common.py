"""Shared pieces of the audio front-end tests: a RIFF/WAVE writer, seeded PCM clips, and the float64 reference with its per-output
fp32 error bound."""
from __future__ import annotations

import struct

import numpy as np

from pantomatrix_amd import audio


def write_wav(path, samples, sr, bits=16, tag=1):
    """samples: (n, ch) integer array (tag 1: PCM of `bits` bits) or float array (tag 3) -> a canonical 44-byte-header WAV file."""
    samples = np.asarray(samples)
    n, ch = samples.shape
    if tag == 3:
        body = samples.astype("<f4" if bits == 32 else "<f8").tobytes()
    elif bits == 24:
        v = samples.astype(np.int64) & 0xFFFFFF
        body = np.stack([v & 0xFF, (v >> 8) & 0xFF, (v >> 16) & 0xFF], axis=-1).astype(np.uint8).tobytes()
    elif bits == 8:
        body = samples.astype(np.uint8).tobytes()
    else:
        body = samples.astype({16: "<i2", 32: "<i4"}[bits]).tobytes()
    fmt = struct.pack("<HHIIHH", tag, ch, sr, sr * ch * bits // 8, ch * bits // 8, bits)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 4 + 8 + len(fmt) + 8 + len(body) + (len(body) & 1)) + b"WAVE")
        f.write(b"fmt " + struct.pack("<I", len(fmt)) + fmt)
        f.write(b"data" + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b""))


def pcm_clips(n, ch, seed):
    """(3, n, ch) int16: two clips of seeded integers over the whole int16 range, and one of full-scale alternating +-32767 on every
    channel — the input that maximises sum |h x|."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-32768, 32768, size=(3, n, ch), dtype=np.int64)
    x[2] = (32767 * (1 - 2 * (np.arange(n) & 1)))[:, None]
    return x.astype(np.int16)


def reference_and_bound(x, up, down):
    """x: (n,) float64 mono input (exact).  -> (y float64 = audio.resample_host(x), bound (n_out,)):
    bound[m] = (T_m + 2) * 2^-24 * sum_k |h32[j] x[k]| over the T_m taps output m uses — the fp32 dot-product bound (any summation order, fused or
    not) plus one rounding each for the taps (h -> h32) and the down-mix.  The walk over (j, k) is written out here, independent of the
    product's."""
    half = 10 * max(up, down)
    h32 = audio.resample_filter(up, down).astype(np.float32).astype(np.float64)
    n = len(x)
    n_out = -(-n * up // down)
    m = np.arange(n_out, dtype=np.int64)
    kmax = (m * down + half) // up
    kmin = -(-(m * down - half) // up)                       # j = m down + half - k up <= 2 half
    lo, hi = np.maximum(kmin, 0), np.minimum(kmax, n - 1)
    bound = np.empty(n_out)
    for i in range(n_out):
        k = np.arange(lo[i], hi[i] + 1)
        j = m[i] * down + half - k * up
        bound[i] = (len(k) + 2) * 2.0 ** -24 * np.abs(h32[j] * x[k]).sum()
    return audio.resample_host(x, up, down), bound
