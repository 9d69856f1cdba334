"""Motion hints in the lock-step recording pass on the MI355X (csrc/elementwise.hip: emage_pack_motion_hints; pantomatrix_amd/recordings.py):
* the table-driven packing kernel bit for bit against `ops.pack_motion` on the dense windows the table describes, in every storage dtype,
  on the vector (ld = 344) and the scalar (ld = 337) path, rows outside the store included;
* five recordings with hints in ONE pass against the REFERENCE's own `inference(masked_motion, mask)` at B = 1
  (tests/golden/infer_hints_{F}f_b1.npz, tests/golden/make_golden_hints.py): code indices identical, poses / expressions / trans within
  the project's 1e-3 — the hints reach into seed frames, stop inside a window, cover a tail-only recording, and one recording has none;
* the captured pass against the eager one, a replay with other hints of other prefix lengths on the same graph, a hints=True runner
  without hints against a hints=False runner;
* `test_pass(hint_mask=)` over files on disk."""
import json
import os

import numpy as np
import pytest
import torch

import clip_store_common as cc
import common
import fake_hint_ops
from pantomatrix_amd import motion_io, ops, recordings as R, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-3                                               # the project's parity tolerance (test_recordings_gpu.py)
FRAMES = (70, 310, 40, 129, 64)                          # the recordings of test_recordings_gpu.py, input order
FRAMES_OUT = (70, 310, 40, 129, 60)
C = 337


# ---- the kernel --------------------------------------------------------------------------------------------------------------------------
DTYPES = {"f32": lambda: ops.F32, "bf16": lambda: ops.BF16, "h2": lambda: ops.H2, "h2_shift3": lambda: ops.h2_shifted(3)}


def store(rows, ld, seed=0):
    """A hint store of `rows` rows with pitch ld: random motion, random 0 / 1 flags; the padding columns hold values a reader of them would
    show (motion 1e30, flags 0)."""
    g = torch.Generator().manual_seed(seed)
    motion = torch.full((rows, ld), 1e30)
    keep = torch.zeros(rows, ld, dtype=torch.uint8)
    motion[:, :C] = torch.randn(rows, C, generator=g)
    keep[:, :C] = torch.randint(0, 2, (rows, C), generator=g).to(torch.uint8)
    return motion, keep


def bits(x):
    return x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32)


def both(dtype, motion, keep, table, t, seed, emb):
    """-> (the kernel's operand, `ops.pack_motion` on the dense windows the table describes, status)."""
    dense_motion, dense_mask = fake_hint_ops.dense_windows(motion[:, :C], keep[:, :C], torch.tensor(table, dtype=torch.int64), t)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    dm, dk = motion.to(DEV), keep.to(DEV)
    sd = None if seed is None else seed.to(DEV)
    got = ops.pack_motion_hints(dtype, dm[:, :C], dk[:, :C], torch.tensor(table, dtype=torch.int64, device=DEV), emb, 344, t, status, seed=sd)
    want = ops.pack_motion(dtype, dense_motion.to(DEV), dense_mask.to(DEV), emb, 344, seed=sd)
    return got, want, int(status)


@pytest.mark.parametrize("seeded", [False, True])
@pytest.mark.parametrize("ld", [344, 337])
@pytest.mark.parametrize("name", list(DTYPES))
def test_kernel_equals_pack_motion_on_the_dense_windows(name, ld, seeded):
    dtype = DTYPES[name]()
    g = torch.Generator().manual_seed(11)
    emb = torch.randn(C, generator=g).to(DEV)
    motion, keep = store(40, ld)
    t = 9
    seed = torch.randn(3, 4, C, generator=g) if seeded else None
    # first rows at odd offsets; avail 0, 1, 4 (= pre), 5, T; (31, 9) ends in the last row of the store
    for table in ([[1, 0], [13, 1], [27, 4]], [[5, 5], [31, 9], [39, 1]]):
        got, want, status = both(dtype, motion, keep, table, t, seed, emb)
        assert status == 0 and got.shape == (3 * t, 344) and got.dtype == want.dtype
        assert torch.equal(bits(got), bits(want)), (name, ld, seeded, table)
    # one frame, one row
    for table in ([[39, 1]], [[7, 0]]):
        got, want, status = both(dtype, motion, keep, table, 1, None if seed is None else seed[:1, :1], emb)
        assert status == 0 and got.shape == (1, 344) and torch.equal(bits(got), bits(want)), (name, ld, seeded, table)


@pytest.mark.parametrize("ld", [344, 337])
@pytest.mark.parametrize("name", ["f32", "h2"])
def test_kernel_reads_nothing_for_a_row_outside_the_store(name, ld):
    """Table rows the host would never build (no host check stands between `ops.pack_motion_hints` and the kernel): the kernel's own guard
    turns each into a row without hints and reports it; the rows inside the store are still right."""
    dtype = DTYPES[name]()
    g = torch.Generator().manual_seed(12)
    emb = torch.randn(C, generator=g).to(DEV)
    motion, keep = store(40, ld, seed=1)
    seed = torch.randn(7, 4, C, generator=g)
    t = 9
    bad = [[35, 9], [3, 5], [-1, 2], [0, 10], [2, -1], [2 ** 62, 1], [31, 9]]        # rows 1 and 6 lie inside
    as_read = [[0, 0], [3, 5], [0, 0], [0, 0], [0, 0], [0, 0], [31, 9]]
    got, _want, status = both(dtype, motion, keep, bad, t, seed, emb)
    want, _w, clean = both(dtype, motion, keep, as_read, t, seed, emb)
    assert status == 4 and clean == 0
    assert torch.equal(bits(got), bits(want))


# ---- the five recordings against the reference -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models():
    return {p: common.product_models(precision=p, device=DEV) for p in ("fp32", "f16x3")}


def five_waves(seed=1234):
    return [synthetic.synthetic_audio(1, synthetic.samples_for_frames(f), seed=seed)[0] for f in FRAMES]


def golden_hints(golden_dir):
    motions, masks = [], []
    for f in FRAMES:
        g = np.load(os.path.join(golden_dir, f"infer_hints_{f}f_b1.npz"))
        motions.append(g["hint_motion"] if bool(g["has_motion"]) else None)
        masks.append(g["hint_keep"] if bool(g["has_mask"]) else None)
    return motions, masks


def hint_values(frames, seed):
    g = torch.Generator().manual_seed(seed)
    aa = 0.2 * torch.randn(frames, 55, 3, generator=g)
    return torch.cat([R.axis_angle_to_rot6d(aa).reshape(frames, 330), 0.05 * torch.randn(frames, 3, generator=g),
                      torch.randint(0, 2, (frames, 4), generator=g).float()], dim=-1).numpy()


def other_hints():
    """Other hints of other prefix lengths for the same five lengths: where the goldens' set has hints this one has none, and the reverse."""
    ones = lambda f: np.ones((f, C), np.uint8)
    m310, m40, m129, m64 = ones(100), ones(40), ones(129), ones(64)
    m310[:, R.part_columns("hands")] = 0
    m40[:, R.part_columns("lower")] = 0
    m129[100:, R.part_columns("upper")] = 0
    m64[[10, 61]] = 0
    return ([None, hint_values(100, 21), hint_values(40, 22), hint_values(129, 23), hint_values(64, 24)], [None, m310, m40, m129, m64])


def run(runner, rs):
    results = [tuple(a.copy() for a in r) for r in runner(rs)]
    codes = [{k: v.cpu().numpy().copy() for k, v in runner.codes_of(i).items()} for i in range(len(FRAMES))]
    return results, codes


@pytest.fixture(scope="module")
def eager(models, golden_dir):
    """The five hinted recordings through an EAGER runner per precision -> {precision: (runner, results, codes)}; computed once, read-only."""
    motions, masks = golden_hints(golden_dir)
    out = {}
    for p, (model, vq) in models.items():
        rs = R.RecordingSet.from_audio(five_waves(), DEV, masked_motion=motions, mask=masks)
        runner = R.RecordingRunner.for_set(model, vq, rs, use_graph=False)
        assert runner.hints and runner.seeded
        out[p] = (runner,) + run(runner, rs)
    return out


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("k", range(len(FRAMES)))
def test_hinted_pass_matches_the_reference_goldens(eager, golden_dir, precision, k):
    _runner, results, codes = eager[precision]
    g = np.load(os.path.join(golden_dir, f"infer_hints_{FRAMES[k]}f_b1.npz"))
    assert float(g["gap_logit"]) >= float(g["gap_logit_unhinted"]) and float(g["gap_distance"]) >= float(g["gap_distance_unhinted"])
    poses, expressions, trans = results[k]
    assert poses.shape == (FRAMES_OUT[k], 165) and g["poses"].shape == (1, FRAMES_OUT[k], 165)
    for p in ("face", "upper", "hands", "lower"):
        assert np.array_equal(codes[k][p], g[f"index_{p}"][0]), f"{FRAMES[k]} frames: {p} code indices differ"
    for nm, got in (("poses", poses), ("expressions", expressions), ("trans", trans)):
        err = float(np.abs(got - g[nm][0]).max())
        print(f"{precision} hinted {FRAMES[k]}f {nm}: max|err| {err:.2e}")
        assert err < TOL, (nm, err)
    if FRAMES[k] == 129:                                                           # no hints of its own: what it generates alone
        plain = np.load(os.path.join(golden_dir, "infer_129f_b1.npz"))
        for p in ("face", "upper", "hands", "lower"):
            assert np.array_equal(codes[k][p], plain[f"index_{p}"][0]), p


# ---- the graph ---------------------------------------------------------------------------------------------------------------------------
def equal_results(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for ra, rb in zip(a, b) for x, y in zip(ra, rb))


@pytest.fixture(scope="module")
def captured(models, golden_dir):
    model, vq = models["f16x3"]
    motions, masks = golden_hints(golden_dir)
    rs = R.RecordingSet.from_audio(five_waves(), DEV, masked_motion=motions, mask=masks)
    return R.RecordingRunner.for_set(model, vq, rs, use_graph=True), rs


def test_captured_pass_equals_the_eager_pass(captured, eager):
    runner, rs = captured
    assert runner.graph is not None and runner.hints
    assert equal_results(runner(rs), eager["f16x3"][1])
    assert equal_results(runner(), eager["f16x3"][1])                              # a replay on the same inputs


def test_replay_with_other_hints_needs_no_new_graph(captured, eager, models):
    model, vq = models["f16x3"]
    runner, rs = captured
    graph = runner.graph
    motions, masks = other_hints()
    other = R.RecordingSet.from_audio(five_waves(), DEV, masked_motion=motions, mask=masks)
    assert other.hint_len == [0, 100, 40, 129, 64] and rs.hint_len == [70, 200, 10, 0, 20]
    got = [tuple(a.copy() for a in r) for r in runner(other)]
    fresh = R.RecordingRunner.for_set(model, vq, other, use_graph=False)           # its store never saw the first set
    want = fresh(other)
    assert runner.graph is graph
    assert equal_results(got, want) and not equal_results(got, eager["f16x3"][1])
    assert equal_results(runner(rs), eager["f16x3"][1]) and runner.graph is graph  # and back


def test_hints_runner_without_hints_equals_the_plain_runner(captured, models):
    model, vq = models["f16x3"]
    runner, rs = captured
    plain = R.RecordingSet.from_audio(five_waves(), DEV)
    assert not plain.hinted and plain.hint_len == [0] * 5
    base = R.RecordingRunner.for_set(model, vq, plain, use_graph=False)
    assert not base.hints
    want = [tuple(a.copy() for a in r) for r in base(plain)]
    assert equal_results(runner(plain), want)                                      # the store still holds the last set's rows: no table row reaches them
    with pytest.raises(ValueError, match="hints=True"):
        base.load(rs)


# ---- files -------------------------------------------------------------------------------------------------------------------------------
def test_test_pass_with_a_hint_mask_over_files(models, tmp_path):
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
    with open(index, "w") as f:
        json.dump(items, f)

    def upper_body(item, frames):
        if item["video_id"] == "rec2_2":
            return None                                                            # this recording is generated from its seed alone
        mask = np.ones((frames, C), np.uint8)
        mask[:, R.part_columns("upper")] = 0
        return mask
    rs0 = R.RecordingSet.from_index(index, "test", DEV, hint_mask=upper_body)
    assert rs0.frames == [19, 26, 19, 11, 70] and rs0.hinted and rs0.hint_len == [19, 26, 19, 11, 70]
    assert torch.equal(rs0.seeds, R.RecordingSet.from_index(index, "test", DEV).seeds)
    runner = R.RecordingRunner.for_set(model, vq, rs0, use_graph=False)
    assert runner.hints
    kept = {}

    def keep(rs):
        kept["rs"] = rs
        kept["results"] = [tuple(a.copy() for a in r) for r in runner(rs)]
        return kept["results"]
    keep.device = DEV
    test_list, save_list = R.test_pass(model, vq, [index], str(tmp_path / "out"), runner=keep, hint_mask=upper_body)
    assert kept["rs"].hinted and torch.equal(kept["rs"].hint_keep, rs0.hint_keep) and torch.equal(kept["rs"].hint_motion, rs0.hint_motion)
    assert [e["video_id"] for e in save_list] == [it["video_id"] for it in test_list] == ["rec0_0", "rec1_1", "held_out", "rec2_2", "rec3_3"]
    for e, (poses, expressions, trans), f in zip(save_list, kept["results"], (19, 26, 19, 11, 70)):
        got = motion_io.beat_format_load(e["motion_path"])
        assert got["poses"].shape == (f, 165) and np.array_equal(got["poses"], poses)
        assert np.array_equal(got["expressions"], expressions) and np.array_equal(got["trans"], trans)
        assert np.isfinite(poses).all()
    # the kept upper body steers the pass: without the mask the same files generate other motion, except where the callable gave None
    plain = R.RecordingRunner.for_set(model, vq, R.RecordingSet.from_index(index, "test", DEV), use_graph=False)
    base = plain(R.RecordingSet.from_index(index, "test", DEV))
    differs = [not np.array_equal(b[0], h[0]) for b, h in zip(base, kept["results"])]
    assert not differs[3] and any(differs)


def test_mask_only_hints_through_for_set_match_the_eager_inference(models):
    """`mask` with zeros and no `masked_motion` (the identity pose is given where the mask is 0): `for_set` builds a runner that takes the
    set, and each recording matches the eager B = 1 `inference(mask=)` + decode — codes identical, arrays within the project's 1e-3."""
    model, vq = models["f16x3"]
    waves = [synthetic.synthetic_audio(1, synthetic.samples_for_frames(f))[0] for f in (70, 40)]
    keep = np.ones((31, C), np.uint8)
    keep[2:31, R.part_columns("upper")] = 0                                 # reaches into the seed frames 2 and 3
    keep[20] = 0
    rs = R.RecordingSet.from_audio(waves, DEV, mask=[keep, None])
    assert rs.hinted and rs.seeded
    runner = R.RecordingRunner.for_set(model, vq, rs, use_graph=False)
    assert runner.hints and runner.seeded
    results = runner(rs)
    spk = torch.zeros(1, 1, dtype=torch.long, device=DEV)
    for k, m in enumerate((torch.from_numpy(keep.astype(np.float32)).to(DEV)[None], None)):
        sel = model._select_codes(model.inference(waves[k][None].to(DEV), spk, vq, mask=m))
        pred = vq.decode(**sel, get_global_motion=True, ref_trans=torch.zeros(1, 3, device=DEV))
        codes = runner.codes_of(k)
        for p in ("upper", "hands", "lower"):
            assert torch.equal(codes[p], sel[f"{p}_index"][0]), (k, p)
        for got, key in zip(results[k], ("motion_axis_angle", "expression", "trans")):
            assert float(np.abs(got - pred[key][0].cpu().numpy()).max()) < TOL, (k, key)
