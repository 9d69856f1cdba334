"""On-disk formats either side of the path: BEAT2 npz schema (reference emage_utils/motion_io.py) and WAV input."""
import os
import struct

import numpy as np
import pytest

from pantomatrix_amd import motion_io as mio


def test_npz_schema_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    poses, expr, trans = rng.standard_normal((20, 165), dtype=np.float32), rng.standard_normal((20, 100), dtype=np.float32), rng.standard_normal((20, 3), dtype=np.float32)
    p = str(tmp_path / "clip_output.npz")
    mio.beat_format_save(p, poses, upsample=1, expressions=expr, trans=trans)
    d = np.load(p, allow_pickle=True)
    assert set(d.files) == {"betas", "poses", "expressions", "trans", "model", "gender", "mocap_frame_rate"}
    assert d["betas"].shape == (300,) and d["poses"].shape == (20, 165) and d["expressions"].shape == (20, 100)
    assert str(d["model"]) == "smplx2020" and str(d["gender"]) == "neutral" and int(d["mocap_frame_rate"]) == 30
    back = mio.beat_format_load(p)
    assert np.array_equal(back["poses"], poses) and np.array_equal(back["trans"], trans)
    with pytest.raises(NotImplementedError):
        mio.beat_format_save(p, poses)


def test_mask_select_recover_and_upsample():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((7, 165)).astype(np.float32)
    m = mio.MASK_DICT["local_upper"]
    assert sum(m) == 43 and sum(mio.MASK_DICT["local_full"]) == 54
    sel = mio.select_with_mask(x, m)
    assert sel.shape == (7, 43 * 3)
    rec = mio.recover_from_mask(sel, m)
    keep = np.repeat(np.asarray(m), 3)
    assert np.array_equal(rec[:, keep], x[:, keep]) and not rec[:, ~keep].any()
    up = mio.time_upsample_numpy(x, 2)
    assert up.shape == (14, 165) and np.allclose(up[0], x[0]) and np.allclose(up[-1], x[-1])
    assert np.array_equal(mio.time_upsample_numpy(x, 1), x)


MASKS = ("local_upper", "local_full")
SAVED_ARRAYS = ("betas", "poses", "expressions", "trans")


def reference_inputs():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((9, 165)).astype(np.float32)
    e, t = rng.standard_normal((9, 100)).astype(np.float32), rng.standard_normal((9, 3)).astype(np.float32)
    return x, e, t


def test_formats_match_reference(tmp_path, golden_dir):
    """Same arrays as the reference's numpy helpers produce on the same inputs (tests/golden/make_golden_reference.py recorded them in
    reference_formats.npz)."""
    ref = np.load(os.path.join(golden_dir, "reference_formats.npz"))
    x, e, t = reference_inputs()
    for name in MASKS:
        assert mio.MASK_DICT[name] == [bool(v) for v in ref[f"fmt_mask_{name}"]]
        assert np.array_equal(mio.select_with_mask(x, mio.MASK_DICT[name]), ref[f"fmt_select_{name}"])
        s = ref[f"fmt_select_{name}"]
        assert np.array_equal(mio.recover_from_mask(s, mio.MASK_DICT[name]), ref[f"fmt_recover_{name}"])
    assert np.allclose(mio.time_upsample_numpy(x, 3), ref["fmt_upsample3"], atol=1e-6)
    mio.beat_format_save(str(tmp_path / "a.npz"), x, expressions=e, trans=t, upsample=2)
    a = np.load(tmp_path / "a.npz", allow_pickle=True)
    assert set(a.files) == {str(f) for f in ref["fmt_save_files"]}
    for k in SAVED_ARRAYS:
        b = ref[f"fmt_save_{k}"]
        assert a[k].shape == b.shape and np.allclose(a[k], b, atol=1e-6)


def test_wav_reader(tmp_path):
    sr, n = 16000, 1600
    t = np.arange(n) / sr
    sig = 0.5 * np.sin(2 * np.pi * 440 * t)
    pcm = (sig * 32767).astype("<i2")
    stereo = np.stack([pcm, pcm], axis=1).reshape(-1)
    def write(path, data, ch, rate, bits, tag=1):
        body = data.tobytes()
        hdr = struct.pack("<4sI4s4sIHHIIHH4sI", b"RIFF", 36 + len(body), b"WAVE", b"fmt ", 16, tag, ch, rate, rate * ch * bits // 8, ch * bits // 8, bits, b"data", len(body))
        open(path, "wb").write(hdr + body)
    write(tmp_path / "mono16.wav", pcm, 1, sr, 16)
    write(tmp_path / "stereo16.wav", stereo, 2, sr, 16)
    write(tmp_path / "f32.wav", sig.astype("<f4"), 1, sr, 32, tag=3)
    write(tmp_path / "mono48k.wav", (0.5 * np.sin(2 * np.pi * 440 * np.arange(3 * n) / 48000) * 32767).astype("<i2"), 1, 48000, 16)
    a, r = mio.load_audio(str(tmp_path / "mono16.wav"))
    assert r == 16000 and a.dtype == np.float32 and a.shape == (n,) and np.abs(a - sig).max() < 1e-4
    assert np.allclose(mio.load_audio(str(tmp_path / "stereo16.wav"))[0], a)
    assert np.abs(mio.load_audio(str(tmp_path / "f32.wav"))[0] - sig).max() < 1e-6
    d = mio.load_audio(str(tmp_path / "mono48k.wav"))[0]
    assert abs(len(d) - n) <= 1 and np.abs(d[100:-100] - sig[100:len(d) - 100]).max() < 5e-3
    open(tmp_path / "fake.wav", "wb").write(b"ID3\x04" + b"\0" * 64)
    with pytest.raises(ValueError):
        mio.load_audio(str(tmp_path / "fake.wav"))
