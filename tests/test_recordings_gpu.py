"""The lock-step test pass on the MI355X (pantomatrix_amd/recordings.py, csrc/recordings.hip):
* `emage_gather_windows` / `emage_copy_segments` bit for bit against numpy slicing, out-of-range rows and untouched gaps included;
* five recordings of different lengths in ONE pass against the REFERENCE's B = 1 goldens (tests/golden/infer_{F}f_b1.npz, made from exactly
  these waveforms with no seed and zero ref_trans): code indices identical, poses / expressions / trans within the project's 1e-3;
* the captured pass against the eager one, a replay on other audio, two recordings of equal length, a replay behind a weight update;
* a seeded pass against the CPU oracle's per-recording `inference(masked_motion=seed)` + decode;
* `test_pass` over files on disk."""
import json
import os

import numpy as np
import pytest
import torch

import clip_store_common as cc
import common
from pantomatrix_amd import motion_io, ops, recordings as R, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-3                                               # the project's parity tolerance (test_parity_gpu.py)
FRAMES = (70, 310, 40, 129, 64)                          # input order; every schedule case (see test_schedule_of_the_five)
FRAMES_OUT = (70, 310, 40, 129, 60)
SPF = 533


# ---- the two kernels ---------------------------------------------------------------------------------------------------------------------
def flat_recordings():
    """Three recordings end to end, drawn from the 16 levels of the clip-store fixture (both ends of the s16 range); odd lengths, so a
    recording starts at an odd or an even sample."""
    rng = np.random.default_rng(3)
    counts = [70 * SPF + 5, 64 * SPF + 1, 66 * SPF + 3]
    flat = cc.AUDIO_LEVELS[rng.integers(0, len(cc.AUDIO_LEVELS), sum(counts))]
    return flat, np.cumsum([0] + counts)


@pytest.mark.parametrize("fmt", ["int16", "float32"])
@pytest.mark.parametrize("frames", [9, 64])
def test_gather_windows_equals_numpy_slicing(frames, fmt):
    flat, first = flat_recordings()
    samples, total = frames * SPF, len(flat)
    # rows of all three recordings at odd and even offsets, the last window of the array, and ONE row outside it (row 3)
    offsets = [int(first[0]), int(first[0]) + 60 * SPF + 1, int(first[1]), -1 if frames == 64 else total - samples + 1, int(first[1]) + 7,
               int(first[2]), int(first[2]) + 3, total - samples]
    src = flat if fmt == "int16" else flat.astype(np.float32) / np.float32(32768.0)
    want = np.stack([np.zeros(samples, np.float32) if not 0 <= o <= total - samples else flat[o:o + samples].astype(np.float32) / np.float32(32768.0)
                     for o in offsets])
    out = torch.full((len(offsets), samples), -7.0, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.gather_windows(torch.from_numpy(src).to(DEV), torch.tensor(offsets, dtype=torch.int64, device=DEV), out, status)
    got = out.cpu().numpy()
    assert int(status) == 1
    assert np.array_equal(got[3], np.zeros(samples, np.float32)), "the out-of-range row is zero-filled"
    for b in range(len(offsets)):
        assert np.array_equal(got[b], want[b]), (b, offsets[b])
    # a strided destination (rows of a wider buffer): the columns behind a row keep their contents
    wide = torch.full((3, samples + 3), -7.0, device=DEV)
    status.zero_()
    ops.gather_windows(torch.from_numpy(src).to(DEV), torch.tensor(offsets[:3], dtype=torch.int64, device=DEV), wide[:, :samples], status)
    assert int(status) == 0 and np.array_equal(wide[:, :samples].cpu().numpy(), want[:3]) and bool((wide[:, samples:] == -7.0).all())


@pytest.mark.parametrize("width", [8, 660])
def test_copy_segments_equals_numpy_slicing(width):
    rng = np.random.default_rng(5)
    if width == 8:
        src, dst = rng.integers(-2**62, 2**62, (100,)), np.full((130,), -7, dtype=np.int64)          # int64 codes
    else:
        src, dst = rng.standard_normal((100, 165)).astype(np.float32), np.full((130, 165), -7.0, dtype=np.float32)
    segments = [(3, 0, 1), (10, 5, 9), (31, 41, 60), (99, 129, 1), (0, 20, 9)]       # lengths 1, 9 and 60; gaps at 1-4, 14-19, 29-40, 101-128
    table, longest = ops.segment_table(segments, 100, 130, DEV)
    want = dst.copy()
    for s, d, n in segments:
        want[d:d + n] = src[s:s + n]
    out = torch.from_numpy(dst).to(DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.copy_segments(torch.from_numpy(src).to(DEV), out, table, width, longest, status)
    assert longest == 60 and int(status) == 0
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(want[1:5], dst[1:5]) and np.array_equal(want[101:129], dst[101:129])      # the gaps still hold the sentinel
    # a table row outside the buffers (the host check bypassed): skipped and reported, the other segment still copied
    bad = torch.tensor([[95, 0, 9], [0, 50, 2]], dtype=torch.int64, device=DEV)
    out2 = torch.from_numpy(dst).to(DEV)
    ops.copy_segments(torch.from_numpy(src).to(DEV), out2, bad, width, 9, status)
    want2 = dst.copy()
    want2[50:52] = src[0:2]
    assert int(status) == 2 and np.array_equal(out2.cpu().numpy(), want2)


# ---- the ragged batch against the reference ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models():
    return {p: common.product_models(precision=p, device=DEV) for p in ("fp32", "f16x3")}


def five_waves(seed=1234):
    return [synthetic.synthetic_audio(1, synthetic.samples_for_frames(f), seed=seed)[0] for f in FRAMES]


@pytest.fixture(scope="module")
def eager(models):
    """The five recordings through an EAGER runner per precision -> {precision: (runner, results, codes)}; computed once, read-only."""
    out = {}
    for p, (model, vq) in models.items():
        rs = R.RecordingSet.from_audio(five_waves(), DEV)
        runner = R.RecordingRunner.for_set(model, vq, rs, use_graph=False)
        results = [tuple(a.copy() for a in r) for r in runner(rs)]
        codes = [{k: v.cpu().numpy().copy() for k, v in runner.codes_of(i).items()} for i in range(len(FRAMES))]
        out[p] = (runner, results, codes)
    return out


def test_schedule_of_the_five(eager):
    runner = eager["fp32"][0]
    s = runner.schedule
    assert s.lengths == list(FRAMES) and s.frames == list(FRAMES_OUT)
    assert [len(ids) for _s, ids in s.steps] == [4, 2, 1, 1, 1]                    # active counts
    assert s.tails == {10: [(0, 60), (1, 300)], 9: [(3, 120)], 40: [(2, 0)]}       # 70 and 310 share a tail length; 40 is tail-only; 64 has none
    assert runner.steps == 5 + 3 and runner.order == [1, 3, 0, 4, 2]


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("k", range(len(FRAMES)))
def test_ragged_batch_matches_the_reference_goldens(eager, golden_dir, precision, k):
    _runner, results, codes = eager[precision]
    g = np.load(os.path.join(golden_dir, f"infer_{FRAMES[k]}f_b1.npz"))
    poses, expressions, trans = results[k]
    assert poses.shape == (FRAMES_OUT[k], 165) and expressions.shape == (FRAMES_OUT[k], 100) and trans.shape == (FRAMES_OUT[k], 3)
    assert g["poses"].shape == (1, FRAMES_OUT[k], 165)
    for p in ("face", "upper", "hands", "lower"):
        assert np.array_equal(codes[k][p], g[f"index_{p}"][0]), f"{FRAMES[k]} frames: {p} code indices differ"
    for nm, got in (("poses", poses), ("expressions", expressions), ("trans", trans)):
        err = float(np.abs(got - g[nm][0]).max())
        print(f"{precision} {FRAMES[k]}f {nm}: max|err| {err:.2e}")
        assert err < TOL, (nm, err)


# ---- the graph ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def captured(models):
    model, vq = models["f16x3"]
    rs = R.RecordingSet.from_audio(five_waves(), DEV)
    return R.RecordingRunner.for_set(model, vq, rs, use_graph=True), rs


def equal_results(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for ra, rb in zip(a, b) for x, y in zip(ra, rb))


def test_captured_pass_equals_the_eager_pass(captured, eager):
    runner, rs = captured
    assert runner.graph is not None
    assert equal_results(runner(rs), eager["f16x3"][1])
    assert equal_results(runner(), eager["f16x3"][1])                              # a replay on the same inputs


def test_replay_on_other_audio_equals_an_eager_run(captured, eager):
    runner, rs = captured
    other = R.RecordingSet.from_audio(five_waves(seed=4321), DEV)
    got = [tuple(a.copy() for a in r) for r in runner(other)]
    want = eager["f16x3"][0](other)
    assert equal_results(got, want) and not equal_results(got, eager["f16x3"][1])
    assert equal_results(runner(rs), eager["f16x3"][1])                            # and back


def test_replay_behind_a_weight_update_sees_the_new_weights(captured, eager, models):
    model, _vq = models["f16x3"]
    runner, rs = captured
    w = dict(model.named_parameters())["face_out_proj.weight"]
    saved = w.detach().clone()
    try:
        with torch.no_grad():
            w.mul_(1.25)                                                           # in place: the version stamp moves, as behind a training step
        got = [tuple(a.copy() for a in r) for r in runner(rs)]
        want = eager["f16x3"][0](rs)
        assert equal_results(got, want) and not equal_results(got, eager["f16x3"][1])
    finally:
        with torch.no_grad():
            w.copy_(saved)
    assert equal_results(runner(rs), eager["f16x3"][1])


def test_equal_lengths_are_not_swapped(models, golden_dir):
    """Two recordings of 70 frames with different audio: each output belongs to its own input, in input order, also after the two trade
    places in a replay."""
    model, vq = models["f16x3"]
    n = synthetic.samples_for_frames(70)
    a, b = synthetic.synthetic_audio(1, n)[0], synthetic.synthetic_audio(1, n, seed=99)[0]
    runner = R.RecordingRunner(model, vq, [n, n], use_graph=True)
    ab = [tuple(x.copy() for x in r) for r in runner(R.RecordingSet.from_audio([a, b], DEV))]
    codes_ab = [{k: v.cpu().numpy().copy() for k, v in runner.codes_of(i).items()} for i in range(2)]
    ba = [tuple(x.copy() for x in r) for r in runner(R.RecordingSet.from_audio([b, a], DEV))]
    codes_ba = [{k: v.cpu().numpy().copy() for k, v in runner.codes_of(i).items()} for i in range(2)]
    g = np.load(os.path.join(golden_dir, "infer_70f_b1.npz"))
    for res, codes in ((ab[0], codes_ab[0]), (ba[1], codes_ba[1])):                # `a` is the golden's waveform wherever it stands
        for p in ("face", "upper", "hands", "lower"):
            assert np.array_equal(codes[p], g[f"index_{p}"][0]), p
        for nm, got in zip(("poses", "expressions", "trans"), res):
            assert float(np.abs(got - g[nm][0]).max()) < TOL, nm
    for p in ("upper", "hands", "lower"):
        assert np.array_equal(codes_ab[1][p], codes_ba[0][p]), p                   # `b` keeps its codes too ...
    assert not np.array_equal(codes_ab[0]["upper"], codes_ab[1]["upper"])          # ... and they are not `a`'s


# ---- seeded pass -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_seeded_pass_matches_the_oracle(models, precision):
    from oracle import emage_oracle as orc
    model, vq = models[precision]
    omodel, ovq = common.oracle_models()
    frames = (70, 129, 40)
    waves = [synthetic.synthetic_audio(1, synthetic.samples_for_frames(f), seed=5 + i)[0] for i, f in enumerate(frames)]
    g = torch.Generator().manual_seed(17)
    aa = 0.2 * torch.randn(3, 4, 55, 3, generator=g)
    seeds = torch.cat([orc.axis_angle_to_rotation_6d(aa).reshape(3, 4, 330), 0.05 * torch.randn(3, 4, 7, generator=g)], dim=-1)
    ref_trans = torch.tensor([[0.25, 0.0, -0.5], [-1.0, 0.5, 0.75], [0.125, -0.25, 2.0]])
    rs = R.RecordingSet.from_audio(waves, DEV, seeds=seeds, ref_trans=ref_trans)
    runner = R.RecordingRunner.for_set(model, vq, rs, use_graph=False)
    assert runner.seeded
    results = runner(rs)
    spk = torch.zeros(1, 1, dtype=torch.long)
    for k, f in enumerate(frames):
        with torch.no_grad():
            ref = omodel.inference(waves[k][None], spk, ovq, masked_motion=seeds[k][None])
            sel = omodel.select_codes(ref)
            rdec = ovq.decode(**sel, get_global_motion=True, ref_trans=ref_trans[k][None])
        codes = runner.codes_of(k)
        for p in ("upper", "hands", "lower"):
            assert torch.equal(codes[p].cpu(), sel[f"{p}_index"][0]), (f, p)
        for nm, got, key in zip(("poses", "expressions", "trans"), results[k], ("motion_axis_angle", "expression", "trans")):
            err = float(np.abs(got - rdec[key][0].numpy()).max())
            print(f"{precision} seeded {f}f {nm}: max|err| {err:.2e}")
            assert got.shape[0] == f and err < TOL, (f, nm, err)
        assert abs(float(results[k][2][0, 0]) - float(ref_trans[k, 0])) < 1e-6 and abs(float(results[k][2][0, 2]) - float(ref_trans[k, 2])) < 1e-6


# ---- files -------------------------------------------------------------------------------------------------------------------------------
def test_test_pass_over_files(models, tmp_path):
    model, vq = models["fp32"]
    recordings, _clips = cc.make_recordings()
    rng = np.random.default_rng(11)
    q = lambda f, w: (rng.integers(-8, 8, (f, w)) / 4.0).astype(np.float32)
    recordings.append(dict(poses=q(70, 165), expressions=q(70, 100), trans=q(70, 3), foot_contact=rng.integers(0, 2, (70, 4)).astype(np.float32),
                           audio=cc.AUDIO_LEVELS[rng.integers(0, len(cc.AUDIO_LEVELS), synthetic.samples_for_frames(70))]))
    index = cc.write_files(str(tmp_path), recordings, [(r, 0, 8) for r in range(4)])
    items = json.load(open(index))
    for it in items:
        it["mode"] = "test"
    items.append(dict(items[1], start_idx=1, end_idx=9))                           # a second item of a video_id: dropped
    with open(index, "w") as f:
        json.dump(items, f)
    kept = {}
    rs0 = R.RecordingSet.from_index(index, "test", DEV)
    assert rs0.frames == [19, 26, 19, 11, 70]                                      # rec0, rec1, held_out (rec0 again), rec2, rec3
    runner = R.RecordingRunner.for_set(model, vq, rs0, use_graph=False)
    assert sorted(runner.schedule.tails) == [10, 11, 19, 26] and len(runner.schedule.steps) == 1

    def keep(rs):
        kept["results"] = [tuple(a.copy() for a in r) for r in runner(rs)]
        return kept["results"]
    keep.device = DEV
    test_list, save_list = R.test_pass(model, vq, [index], str(tmp_path / "out"), runner=keep)
    ids = [it["video_id"] for it in test_list]
    assert ids == ["rec0_0", "rec1_1", "held_out", "rec2_2", "rec3_3"] and [e["video_id"] for e in save_list] == ids
    for e, (poses, expressions, trans), f in zip(save_list, kept["results"], (19, 26, 19, 11, 70)):
        assert e["motion_path"] == str(tmp_path / "out" / f"{e['video_id']}_output.npz")
        got = motion_io.beat_format_load(e["motion_path"])
        assert got["poses"].shape == (f, 165) and np.array_equal(got["poses"], poses)
        assert np.array_equal(got["expressions"], expressions) and np.array_equal(got["trans"], trans)
        assert np.isfinite(poses).all()
    # the two items of recording 0 carry the same audio and seed: the same motion, each under its own name
    assert float(np.abs(kept["results"][0][0] - kept["results"][2][0]).max()) < TOL
    assert abs(float(kept["results"][4][2][0, 0]) - float(recordings[3]["trans"][0, 0])) < 1e-6      # trans starts at the recording's ref_trans
