"""Host side of the audio front end (pantomatrix_amd/audio.py) against scipy, and the ABI of its kernel; no GPU needed."""
import os
import re

import numpy as np
import pytest
from scipy.signal import firwin, resample_poly

import audio_common
from pantomatrix_amd import _lib, audio, motion_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIOS = [(1, 3), (160, 441), (2, 1), (320, 441), (640, 441)]       # 48 000, 44 100, 8 000, 22 050, 11 025 -> 16 000


@pytest.mark.parametrize("up,down", RATIOS)
def test_filter_design_is_scipys_default(up, down):
    half = 10 * max(up, down)
    ref = firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up
    h = audio.resample_filter(up, down)
    assert h.dtype == np.float64 and h.shape == ref.shape
    assert np.abs(h - ref).max() <= 1e-14


@pytest.mark.parametrize("up,down", RATIOS)
@pytest.mark.parametrize("n", [4801, 4411, 37, 1])
def test_polyphase_restatement_matches_resample_poly(up, down, n):
    x = np.random.default_rng(n).standard_normal(n)
    y, ref = audio.resample_host(x, up, down), resample_poly(x, up, down)
    assert y.dtype == np.float64 and len(y) == len(ref) == audio.out_length(n, up, down) == int(np.ceil(n * up / down))
    assert np.abs(y - ref).max() <= 1e-12


@pytest.mark.parametrize("up,down", RATIOS)
def test_phase_rows_round_trip(up, down):
    h = audio.resample_filter(up, down).astype(np.float32)
    rows = audio.pack_taps(h, up)
    pitch = audio.phase_pitch(len(h), up)
    assert rows.dtype == np.float32 and rows.shape == (up, pitch) and pitch % 2 == 1 and pitch >= -(-len(h) // up)
    assert np.array_equal(audio.unpack_taps(rows, len(h)), h)
    for p in (0, up // 2, up - 1):                                   # row p: h[p], h[p + up], ... then zeros
        t = h[p::up]
        assert np.array_equal(rows[p, :len(t)], t) and not rows[p, len(t):].any()
    assert rows.nbytes <= 96 * 1024                                  # EMAGE_AUDIO_TAPS_LDS_BYTES


def test_rate_helpers():
    assert audio.rate_ratio(44100, 16000) == (160, 441) and audio.rate_ratio(48000, 16000) == (1, 3) and audio.rate_ratio(16000, 16000) == (1, 1)
    for rate in (44100, 48000, 8000, 11025, 16000):
        up, down = audio.rate_ratio(rate, 16000)
        for n_samples in (1, 2, 37334, 68267):
            n = audio.AudioInput(rate, 2).frames_for(n_samples)
            assert audio.out_length(n, up, down) >= n_samples and (n == 1 or audio.out_length(n - 1, up, down) < n_samples)
    with pytest.raises(ValueError):
        audio.AudioInput(44100, 2, "u8")


@pytest.mark.parametrize("sr,bits,tag,ch", [(44100, 16, 1, 2), (48000, 24, 1, 1), (16000, 32, 3, 2), (22050, 8, 1, 1)])
def test_loader_without_device_is_motion_io(tmp_path, sr, bits, tag, ch):
    rng = np.random.default_rng(bits)
    if tag == 3:
        x = rng.standard_normal((3001, ch)) * 0.2
    elif bits == 8:
        x = rng.integers(0, 256, size=(3001, ch))
    else:
        x = rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), size=(3001, ch))
    path = str(tmp_path / "clip.wav")
    audio_common.write_wav(path, x, sr, bits, tag)
    got, got_sr = audio.load_audio(path)
    ref, ref_sr = motion_io.load_audio(path)
    assert got_sr == ref_sr == 16000 and got.dtype == np.float32 and np.array_equal(got, ref)
    assert len(got) == audio.out_length(3001, *audio.rate_ratio(sr, 16000))


def test_raw_pcm_of_a_file_is_its_data_chunk(tmp_path):
    """The tensors `load_audio(path, device=...)` uploads: the file's samples undecoded, in the shapes ops.audio_resample takes."""
    import torch
    rng = np.random.default_rng(5)
    for bits, tag, dtype, last in ((16, 1, torch.int16, 2), (24, 1, torch.uint8, 6), (32, 1, torch.int32, 2), (32, 3, torch.float32, 2)):
        x = rng.standard_normal((50, 2)) if tag == 3 else rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), size=(50, 2))
        path = str(tmp_path / f"c{bits}_{tag}.wav")
        audio_common.write_wav(path, x, 44100, bits, tag)
        pcm, ch, sr = audio._pcm_tensor(path)
        assert (pcm.dtype, tuple(pcm.shape), ch, sr) == (dtype, (1, 50, last), 2, 44100)
        if bits != 24:
            assert np.array_equal(pcm[0].numpy(), x.astype(pcm[0].numpy().dtype))
        else:
            b = pcm[0].numpy().reshape(50, 2, 3).astype(np.int64)
            v = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
            assert np.array_equal((v ^ 0x800000) - 0x800000, x)


def test_abi_of_the_audio_entry_point():
    text = open(os.path.join(ROOT, "include", "emage_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int\s+emage_audio_resample\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, "emage_audio_resample is not declared in include/emage_hip.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 14 == len(_lib.SIGNATURES["emage_audio_resample"])
    codes = dict(re.findall(r"#define\s+(EMAGE_(?:PCM_\w+|AUDIO_TILE))\s+(\d+)", text))
    assert codes == {"EMAGE_PCM_S16": str(_lib.PCM_S16), "EMAGE_PCM_S24": str(_lib.PCM_S24), "EMAGE_PCM_S32": str(_lib.PCM_S32),
                     "EMAGE_PCM_F32": str(_lib.PCM_F32), "EMAGE_AUDIO_TILE": str(_lib.AUDIO_TILE)}
    lib = _lib.load()
    assert hasattr(lib, "emage_audio_resample")
    assert _lib.ABI_VERSION == 20 == lib.emage_abi_version()


def test_argument_validation_without_gpu():
    """Every refusal happens before the launch, so it can be exercised here (the pointers are never dereferenced)."""
    import ctypes as C
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    n_taps = 20 * 441 + 1

    def call(fmt=_lib.PCM_S16, pcm=p, pitch=4 * 441, ch=2, n_in=441, taps=p, n_taps=n_taps, up=160, down=441, out=p, ldo=160, n_out=160, clips=1):
        return lib.emage_audio_resample(fmt, pcm, pitch, ch, n_in, taps, n_taps, up, down, out, ldo, n_out, clips, None)

    assert call(pcm=None) == -1 and call(out=None) == -1 and call(taps=None) == -1
    assert call(ch=0) == -1 and call(ch=9) == -1 and call(fmt=4) == -1 and call(fmt=-1) == -1
    assert call(n_out=161) == -1 and call(n_out=159) == -1 and call(ldo=159) == -1
    assert call(pitch=4 * 441 - 2) == -1                            # shorter than one clip
    assert call(n_taps=n_taps - 1) == -1 and call(n_taps=20 * 160 + 1) == -1
    assert call(up=4096, down=4097, n_taps=20 * 4097 + 1, n_out=441, ldo=441) == -1     # 4096 phase rows of 21 floats: beyond the LDS budget
    assert call(up=1, down=64, n_taps=1281, n_in=640, pitch=4 * 640, n_out=10, ldo=10) == -1   # one tile's input span beyond the LDS budget
    assert call(clips=0) == -1 and call(n_in=0, n_out=0) == -1
    assert call(pcm=p + 1) == -1                                     # int16 samples off their alignment
