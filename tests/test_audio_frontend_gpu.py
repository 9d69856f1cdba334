"""The audio front end on the MI355X (emage_audio_resample through ops.audio_resample / audio.load_audio / ClipRunner(audio_input=...)):
decode and down-mix bit-exact against the host reader, resampling against the float64 restatement within the fp32 dot-product bound
computed per output, strided access with canaries, refusals, reproducibility, and the plumbing end to end."""
import functools

import numpy as np
import pytest
import torch

import audio_common
import common
from pantomatrix_amd import _lib, audio, motion_io, ops, synthetic
from pantomatrix_amd.runtime import ClipRunner

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILE = _lib.AUDIO_TILE
RATES = [48000, 44100, 8000, 22050, 11025]


def tile_frame_counts(rate):
    """Frame counts around the kernel's tile: the fewest frames with n_out >= 2 TILE + 1 (three tiles, the last one short; n_out == 2 TILE + 1
    wherever the rate pair reaches it) and the most frames with n_out <= TILE - 1 (one short tile)."""
    up, down = audio.rate_ratio(rate, 16000)
    hi = (2 * TILE) * down // up + 1
    lo = (TILE - 1) * down // up
    assert audio.out_length(hi, up, down) >= 2 * TILE + 1 > audio.out_length(hi - 1, up, down)
    assert audio.out_length(lo, up, down) <= TILE - 1 < audio.out_length(lo + 1, up, down)
    return hi, lo


def encode(x16, fmt):
    """(B, n, ch) int16 clips -> the device tensor of format `fmt` holding the same sample VALUES scaled to the format's width
    (s24 / s32: shifted up, low bits filled from the sample itself so they are not all zero), and the float32 (B, n, ch) the host reader
    decodes from the same bytes."""
    x = x16.astype(np.int64)
    b, n, ch = x.shape
    if fmt == "s16":
        raw, dec = x16, x16.astype(np.float32) / 32768.0
    elif fmt == "s24":
        v = (x << 8) | (x & 0xFF)
        u = v & 0xFFFFFF
        raw = np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=-1).astype(np.uint8).reshape(b, n, ch * 3)
        dec = v.astype(np.float32) / 8388608.0
    elif fmt == "s32":
        v = (x << 16) | (x & 0xFFFF)                      # 31 significant bits: int32 -> float32 has to round
        raw, dec = v.astype(np.int32), v.astype(np.int32).astype(np.float32) / 2147483648.0
    else:
        raw = dec = (x16.astype(np.float32) / 32768.0) * np.float32(1.0001)
    return torch.from_numpy(np.ascontiguousarray(raw)).to(DEV), dec


def host_mono(dec):
    """motion_io.load_audio's down-mix of a decoded (n, ch) float32 clip."""
    return dec.mean(axis=1) if dec.shape[1] > 1 else dec[:, 0]


@pytest.mark.parametrize("fmt", ["s16", "s24", "s32", "f32"])
@pytest.mark.parametrize("ch", [1, 2])
def test_decode_and_downmix_are_exact(tmp_path, fmt, ch):
    x16 = audio_common.pcm_clips(4411, ch, seed=ch)
    pcm, dec = encode(x16, fmt)
    got = ops.audio_resample(pcm, ch, 16000, 16000)
    want = torch.from_numpy(np.stack([host_mono(d) for d in dec]))
    assert got.shape == (3, 4411) and torch.equal(got.cpu(), want)
    # ... and the decode above IS the host reader's: one clip through a file
    bits, tag = {"s16": (16, 1), "s24": (24, 1), "s32": (32, 1), "f32": (32, 3)}[fmt]
    path = str(tmp_path / "clip.wav")
    file_samples = {"s16": x16[0], "s24": (x16[0].astype(np.int64) << 8) | (x16[0] & 0xFF), "s32": (x16[0].astype(np.int64) << 16) | (x16[0].astype(np.int64) & 0xFFFF),
                    "f32": dec[0]}[fmt]
    audio_common.write_wav(path, file_samples, 16000, bits, tag)
    ref, _ = motion_io._read_wav(path)
    assert np.array_equal(ref, dec[0])
    dev_audio, sr = audio.load_audio(path, device=DEV)
    assert sr == 16000 and torch.equal(dev_audio.cpu(), torch.from_numpy(motion_io.load_audio(path)[0]))


def test_six_channel_downmix_within_2_ulp():
    x16 = audio_common.pcm_clips(4411, 6, seed=6)
    x16[:, :, 1::2] //= 3                                   # unequal channels: the order of the sum matters
    pcm, dec = encode(x16, "s16")
    got = ops.audio_resample(pcm, 6, 16000, 16000).cpu().numpy()
    want = np.stack([host_mono(d) for d in dec])
    ulp = np.spacing(np.abs(want).astype(np.float32))
    assert (np.abs(got.astype(np.float64) - want) <= 2 * ulp).all()


@functools.lru_cache(maxsize=None)
def resample_case(rate, ch, n):
    """Seeded int16 clips, and per clip the float64 reference with its bound (computed once per case)."""
    x16 = audio_common.pcm_clips(n, ch, seed=rate + 7 * ch + n)
    up, down = audio.rate_ratio(rate, 16000)
    mono = x16.astype(np.float64).mean(axis=2) / 32768.0          # exact in float64
    return x16, [audio_common.reference_and_bound(m, up, down) for m in mono]


def assert_within_bound(got, refs, what):
    for b, (ref, bound) in enumerate(refs):
        err = np.abs(got[b].astype(np.float64) - ref)
        worst = int(np.argmax(err - bound))
        print(f"{what} clip {b}: max|err| {err.max():.3e}, bound {bound.min():.3e}..{bound.max():.3e}, closest at m={worst}: {err[worst]:.3e} vs {bound[worst]:.3e}")
        assert err.shape == bound.shape and (err <= bound).all(), (what, b, worst, float(err[worst]), float(bound[worst]))


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("ch", [1, 2])
def test_resampling_matches_float64_within_the_fp32_bound(rate, ch):
    up, down = audio.rate_ratio(rate, 16000)
    for n in (4411, 37, 1) + tile_frame_counts(rate):
        x16, refs = resample_case(rate, ch, n)
        got = ops.audio_resample(torch.from_numpy(x16).to(DEV), ch, rate)
        assert got.shape == (3, audio.out_length(n, up, down)) and got.dtype == torch.float32
        assert_within_bound(got.cpu().numpy(), refs, f"{rate} Hz x{ch} n={n}")


@pytest.mark.parametrize("rate", RATES)
def test_dc_gain(rate):
    """A constant 1.0 comes out as the DC gain of the phase that output uses, sum_i h[p + i up], within the bound, at every output whose
    taps all meet input: farther than the filter's reach + 1 from either end — half / up input frames, which is half / down outputs (more
    than half / up when up > down; the float64 reference is asserted to be clear of the ends over the same range).  For up == 1 that gain is 1 (the filter has unit DC gain): the output is 1.0 within the bound.  For
    up > 1 the polyphase branches of the Kaiser design do not each sum to one — scipy.signal.resample_poly itself returns 1 -+ 5.9e-5 for
    160 / 441 and 1 -+ 6.8e-4 for 640 / 441 in float64 — so there the yardstick is the float64 branch sum, and 1.0 within that ripple."""
    up, down = audio.rate_ratio(rate, 16000)
    n, half = 4411, 10 * max(up, down)
    ones = np.ones(n)
    ref, bound = audio_common.reference_and_bound(ones, up, down)
    got = ops.audio_resample(torch.ones(3, n, 1, device=DEV), 1, rate).cpu().numpy().astype(np.float64)
    reach = max(half // up, -(-half // down)) + 2
    inner = slice(reach, len(ref) - reach)
    assert len(ref[inner]) > 100
    h = audio.resample_filter(up, down)
    gain = np.array([h[p::up].sum() for p in range(up)])[(np.arange(len(ref)) * down + half) % up]
    ripple = np.abs(gain - 1).max()
    print(f"{rate} Hz: max|y - 1| {np.abs(got[:, inner] - 1).max():.3e}, max|y - branch gain| {np.abs(got[:, inner] - gain[inner]).max():.3e}, "
          f"bound {bound[inner].max():.3e}, float64 branch ripple {ripple:.3e}")
    assert np.abs(ref[inner] - gain[inner]).max() < 1e-13
    assert (np.abs(got[:, inner] - gain[inner]) <= bound[inner]).all()
    if up == 1:
        assert ripple < 1e-15 and (np.abs(got[:, inner] - 1.0) <= bound[inner]).all()
    else:
        assert (np.abs(got[:, inner] - 1.0) <= bound[inner] + ripple).all()


@pytest.mark.parametrize("rate,ch,fmt,pad", [(44100, 2, "s16", 5), (44100, 2, "s16", 3), (48000, 1, "s16", 5), (48000, 1, "s16", 3), (44100, 2, "s24", 5),
                                             (16000, 2, "s16", 5)])
def test_strided_rows_and_canaries(rate, ch, fmt, pad):
    """PCM rows with a pitch beyond one clip (int16 with pad 5: still 16-byte aligned, the 16-byte loads; pad 3: the per-sample loads), output
    rows with ldo > n_out: the same bits as the contiguous call, and nothing written outside the n_out columns."""
    n = 4411
    x16 = audio_common.pcm_clips(n, ch, seed=3)
    pcm, _ = encode(x16, fmt)
    want = ops.audio_resample(pcm, ch, rate)
    n_out = want.shape[1]
    wide = torch.zeros(3, n + pad, pcm.shape[2], dtype=pcm.dtype, device=DEV)
    wide[:, :n] = pcm
    wide[:, n:] = 77                                        # frames past the clip must not be read as audio
    canary = -12345.678
    buf = torch.full((3 * (n_out + 9) + 64,), canary, dtype=torch.float32, device=DEV)
    out = buf[:3 * (n_out + 9)].view(3, n_out + 9)[:, :n_out]
    got = ops.audio_resample(wide[:, :n], ch, rate, out=out)
    assert got.data_ptr() == out.data_ptr() and torch.equal(got, want)
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[:3 * (n_out + 9)].view(3, n_out + 9)[:, :n_out] = False
    assert torch.equal(buf[mask], torch.full_like(buf[mask], canary))


def test_invalid_arguments_raise_without_launching():
    pcm = torch.zeros(3, 441, 2, dtype=torch.int16, device=DEV)
    canary = torch.full((3, 200), 5.0, device=DEV)
    with pytest.raises(_lib.EmageKernelError, match="EMAGE_EINVAL"):          # wrong n_out (160)
        ops.audio_resample(pcm, 2, 44100, out=canary[:, :161])
    with pytest.raises(_lib.EmageKernelError, match="EMAGE_EINVAL"):
        ops.audio_resample(pcm, 2, 44100, out=canary[:, :159])
    with pytest.raises(_lib.EmageKernelError, match="EMAGE_EINVAL"):          # channels = 0
        ops.audio_resample(pcm, 0, 44100, out=canary[:, :160])
    with pytest.raises(_lib.EmageKernelError, match="EMAGE_EINVAL"):          # ldo = 159 < n_out
        ops.audio_resample(pcm, 2, 44100, out=canary.view(-1).as_strided((3, 160), (159, 1)))
    with pytest.raises(_lib.EmageKernelError, match="EMAGE_EINVAL"):          # 1 : 64 — one tile's input span beyond the LDS budget
        ops.audio_resample(torch.zeros(1, 640, 1, dtype=torch.int16, device=DEV), 1, 64 * 16000, 16000)
    torch.cuda.synchronize()
    assert torch.equal(canary, torch.full_like(canary, 5.0))
    assert ops.audio_resample(pcm, 2, 44100, out=canary[:, :160]).abs().max() == 0      # the valid call goes through


def test_two_launches_give_the_same_bits():
    x16, _ = resample_case(44100, 2, tile_frame_counts(44100)[0])
    pcm = torch.from_numpy(x16).to(DEV)
    a, b = ops.audio_resample(pcm, 2, 44100), ops.audio_resample(pcm, 2, 44100)
    assert torch.equal(a, b)
    taps = audio.packed_taps(160, 441, DEV)
    assert taps is audio.packed_taps(160, 441, pcm.device) and taps.shape == (160, 57) and taps.dtype == torch.float32


def test_wav_to_motion_end_to_end(tmp_path):
    """70 frames, 2 clips, 44.1 kHz stereo 16-bit files: the device loader against the host loader (length, waveform within the bound), and
    ClipRunner(audio_input=...) fed the raw PCM against a default ClipRunner fed the front end's own output — the same bits, eager and as
    a captured graph replayed twice (plumbing only: the numerical claim is the waveform's)."""
    model, vq = common.product_models(precision="f16x3", device=DEV)
    n_samples = synthetic.samples_for_frames(70)
    spec = audio.AudioInput(44100, 2, "s16")
    n_in = spec.frames_for(n_samples)
    rng = np.random.default_rng(70)
    x16 = np.clip(np.rint(0.1 * 32768 * rng.standard_normal((2, n_in, 2))), -32768, 32767).astype(np.int16)
    waves = []
    for b in range(2):
        path = str(tmp_path / f"clip{b}.wav")
        audio_common.write_wav(path, x16[b], 44100, 16)
        host, sr = motion_io.load_audio(path)
        dev_audio, dev_sr = audio.load_audio(path, device=DEV)
        assert sr == dev_sr == 16000 and dev_audio.shape == host.shape == (n_samples,) and dev_audio.dtype == torch.float32
        ref, bound = audio_common.reference_and_bound(x16[b].astype(np.float64).mean(axis=1) / 32768.0, 160, 441)
        # the host loader rounds its float64 result to float32: at most one more ulp of it on top of the bound
        assert (np.abs(dev_audio.cpu().numpy().astype(np.float64) - host) <= bound + np.spacing(np.abs(host))).all()
        assert_within_bound(dev_audio.cpu().numpy()[None], [(ref, bound)], f"clip {b}")
        waves.append(dev_audio)
    pcm = torch.from_numpy(x16).to(DEV)
    front = ops.audio_resample(pcm, 2, 44100)[:, :n_samples]
    assert torch.equal(front, torch.stack(waves))
    want = [torch.from_numpy(x.copy()) for x in ClipRunner(model, vq, 2, n_samples, use_graph=False)(front)]
    for use_graph in (False, True):
        fed = ClipRunner(model, vq, 2, n_samples, use_graph=use_graph, audio_input=spec)
        assert fed.n_in == n_in and tuple(fed.pcm.shape) == (2, n_in, 2) and fed.pcm.dtype == torch.int16
        for _ in range(2 if use_graph else 1):
            got = [torch.from_numpy(x.copy()) for x in fed(pcm)]
            assert got[0].shape == (2, 70, 165) and len(got) == 3
            for g, w in zip(got, want):
                assert torch.equal(g, w)
        fed(torch.zeros_like(pcm))                           # another batch in between: the replay really reads its input
        got = [torch.from_numpy(x.copy()) for x in fed(pcm)]
        assert all(torch.equal(g, w) for g, w in zip(got, want))


def test_runner_reads_a_longer_resampled_row_in_place():
    """8 kHz mono, odd n_samples: every frame count gives an even n_out, so the resampled rows are one sample longer than n_samples and
    the models read a row-strided view of them.  Same bits as a default runner fed that view's content; eager, one window and a tail."""
    model, vq = common.product_models(precision="f16x3", device=DEV)
    n_samples = synthetic.samples_for_frames(70) + 1
    assert n_samples % 2 == 1 and n_samples * 30 // 16000 == 70
    spec = audio.AudioInput(8000, 1, "s16")
    fed = ClipRunner(model, vq, 2, n_samples, use_graph=False, warmup=1, audio_input=spec)
    assert fed._resampled.shape[1] == n_samples + 1 == 2 * fed.n_in and fed.audio.stride(0) == n_samples + 1 and fed.audio.shape == (2, n_samples)
    rng = np.random.default_rng(8)
    pcm = torch.from_numpy(np.clip(np.rint(0.1 * 32768 * rng.standard_normal((2, fed.n_in, 1))), -32768, 32767).astype(np.int16)).to(DEV)
    front = ops.audio_resample(pcm, 1, 8000)[:, :n_samples].contiguous()
    want = ClipRunner(model, vq, 2, n_samples, use_graph=False, warmup=1)(front)
    got = fed(pcm)
    assert got[0].shape == (2, 70, 165)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
