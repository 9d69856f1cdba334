"""Per-clip speaker ids on the MI355X: `emage_embedding_backward` against a float64 `index_add_`, one eager and one captured training step
with four speakers against the REAL reference step (tests/golden/train_step_speakers.npz), the loader's `speaker_id` buffer and a captured
step fed by it, `validation.Validator` with ids, and `recordings.RecordingRunner` with one id per recording."""
import numpy as np
import pytest
import torch

import common
import speaker_common as sc
from pantomatrix_amd import data, ops, recordings as R, synthetic, training, validation

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---- 5. the kernel ---------------------------------------------------------------------------------------------------------------------
def _embedding_case(b, t, d, s, ids, strided):
    gen = torch.Generator().manual_seed(b * 1000 + d)
    pad = 3 if strided else 0
    big_g = torch.randn(b * t, d + pad, generator=gen).to(DEV)
    g = big_g[:, :d]
    big_dw = torch.full((s, d + pad), -7.0, device=DEV)
    ids = torch.tensor(ids, dtype=torch.int64, device=DEV)
    return g, ids, big_dw, big_dw[:, :d]


def _reference(g, ids, s, t):
    """float64: per clip the sum over its T rows, then index_add_ over the clamped ids; with it the sum of |g| per table row (the bound)."""
    b, d = ids.numel(), g.shape[1]
    k = ids.clamp(0, s - 1).cpu()
    g64 = g.double().cpu().reshape(b, t, d)
    ref = torch.zeros(s, d, dtype=torch.float64).index_add_(0, k, g64.sum(1))
    mag = torch.zeros(s, d, dtype=torch.float64).index_add_(0, k, g64.abs().sum(1))
    return ref, mag, k


CASES = {
    "one": (1, 1, 1, 1, [0], False),
    "strided_unused_row": (5, 3, 70, 4, [3, 0, 3, 1, 3], True),
    "model_shape": (7, 64, 768, 3, [2, 0, 1, 1, 2, 0, 2], False),
    "many_clips": (300, 2, 257, 5, [(7 * i) % 5 for i in range(300)], False),
}


@pytest.mark.parametrize("case", list(CASES))
def test_embedding_backward_against_float64(case):
    """|got - ref| <= 2^-24 |ref| + n 2^-52 sum|g| per element, n = B * T: the kernel adds exactly representable values in float64 (each add
    rounds by at most 2^-53 of the running magnitude, itself at most sum|g|) and rounds to fp32 once (2^-24 |ref|).  Rows no clip names are
    exactly 0.0; two runs give the same bits; a strided destination keeps the columns behind its rows."""
    b, t, d, s, ids, strided = CASES[case]
    g, ids, big_dw, dw = _embedding_case(b, t, d, s, ids, strided)
    got = ops.embedding_backward(g, ids, s, dw=dw)
    ref, mag, k = _reference(g, ids, s, t)
    err = (got.double().cpu() - ref).abs()
    bound = 2.0 ** -24 * ref.abs() + (b * t) * 2.0 ** -52 * mag
    print(f"{case}: max err {float(err.max()):.3e}, largest err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all()), (case, float((err - bound).max()))
    unused = sorted(set(range(s)) - set(k.tolist()))
    if case == "strided_unused_row":
        assert unused == [2]
    for row in unused:
        assert bool((got[row] == 0.0).all()) and not bool(torch.signbit(got[row]).any()), row
    if strided:
        assert bool((big_dw[:, d:] == -7.0).all()), "columns behind the rows of a strided destination were written"
    again = ops.embedding_backward(g, ids, s)
    assert torch.equal(again, got)
    assert ops.embedding_backward(g, ids, s, dw=torch.full_like(again, 5.0)).equal(got), "the kernel writes, it does not accumulate"


def test_embedding_backward_clamps_as_the_forward_gather_does():
    g = torch.randn(3 * 4, 33, generator=torch.Generator().manual_seed(2)).to(DEV)
    raw = ops.embedding_backward(g, torch.tensor([-1, 5, 1], dtype=torch.int64, device=DEV), 3)
    clamped = ops.embedding_backward(g, torch.tensor([0, 2, 1], dtype=torch.int64, device=DEV), 3)
    assert torch.equal(raw, clamped)
    table = torch.randn(3, 33, generator=torch.Generator().manual_seed(3)).to(DEV)
    sid = torch.tensor([[-1], [5], [1]], dtype=torch.int64, device=DEV).expand(3, 4)
    assert torch.equal(ops.gather_rows(table, sid, ops.F32).view(3, 4, 33)[:, 0], table[[0, 2, 1]])      # the forward used exactly those rows


# ---- 6. one eager step against the reference -------------------------------------------------------------------------------------------
def _step_inputs(g):
    r = sc.oracle_step(g)
    batch = {k: v.to(DEV) for k, v in r["batch"].items()}
    masks = [[m.to(DEV).contiguous() for m in fm] for fm in r["masks"]]
    return batch, masks, r["random_mask"].to(DEV), torch.from_numpy(g["speaker_ids"]).reshape(-1, 1)


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_training_step_with_speaker_ids_matches_the_reference(golden_dir, precision):
    """The bars of test_training_step_matches_the_reference_in_losses_gradient_norms_and_parameter_sums on the four-speaker golden, plus every
    ROW of the two speaker tables' gradients (norm within 5e-3 relative; the unused row exactly zero, its parameters untouched)."""
    g = sc.golden(golden_dir)
    batch, masks, random_mask, ids = _step_inputs(g)
    model, vq = sc.product_models(int(g["speaker_dims"]), precision=precision, device=DEV)
    before = {k: v.clone() for k, v in model._flat_params().items()}
    trainer = training.Trainer(model, vq)
    seen = {}
    losses = trainer.step(batch, int(g["iteration"]), masks, random_mask, speaker_id=ids,
                          grad_hook=lambda gr: seen.update({k: v.clone() for k, v in gr.items()}))
    for k in sc.LOSS_KEYS:
        want = float(g["loss_" + k])
        print(f"{precision} {k}: {losses[k]:.6f} reference {want:.6f}")
        assert abs(losses[k] - want) < 2e-4 * max(1.0, abs(want)), k
    names = [str(n) for n in g["grad_names"]]
    gmax = float(np.max(g["grad_norms"]))
    params = model._flat_params()
    checked, lr = 0, 1.5e-4
    for n, norm, first, shadowed, s in zip(names, g["grad_norms"], g["grad_first"], g["shadowed"], g["param_sum_after"]):
        assert n in seen, n
        if shadowed:
            continue
        wav = n.startswith(("audio_encoder_face.", "audio_encoder_body."))
        gn = float(seen[n].norm())
        assert abs(gn - float(norm)) <= (3e-2 if wav else 5e-3) * float(norm) + 1e-6 * gmax, (n, gn, float(norm))
        if not wav:
            assert abs(float(seen[n].reshape(-1)[0]) - float(first)) <= 5e-3 * float(seen[n].abs().max()) + 1e-6 * gmax, n
        p = params[n]
        assert abs(float(p.double().sum()) - float(s)) <= 3e-5 * p.numel() ** 0.5 + 2e-3 + (0.3 * lr * p.numel() if wav else 0), n
        assert not torch.equal(p, before[n]), n
        checked += 1
    assert checked > 440
    for n in sc.TABLES:
        want = torch.from_numpy(g["grad/" + n])
        got = seen[n].reshape(want.shape).cpu()
        for row in range(3):
            rn, wn = float(got[row].norm()), float(want[row].norm())
            print(f"{precision} {n} row {row}: norm {rn:.6f} reference {wn:.6f}, |diff| / |ref| {float((got[row] - want[row]).norm()) / wn:.2e}")
            assert abs(rn - wn) <= 5e-3 * wn, (n, row)                       # the rows' norms lie 3 % and more apart: a swap would show
        assert float(want[3].abs().max()) == 0.0 and float(got[3].abs().max()) == 0.0, n
        assert torch.equal(params[n][3], before[n][3]) and not torch.equal(params[n][2], before[n][2]), n


def test_eager_step_validates_host_ids(golden_dir):
    g = sc.golden(golden_dir)
    batch, masks, random_mask, _ids = _step_inputs(g)
    model, vq = sc.product_models(int(g["speaker_dims"]), precision="fp32", device=DEV)
    trainer = training.Trainer(model, vq)
    before = {k: v.clone() for k, v in model._flat_params().items()}
    with pytest.raises(ValueError, match="speaker_dims"):
        trainer.step(batch, 0, masks, random_mask, speaker_id=torch.tensor([0, 1, 4, 0]))
    with pytest.raises(RuntimeError, match="speaker_id"):
        trainer.capture(batch, random_mask, masks, speaker_id=torch.tensor([0, 1, 2, 0]))      # a host tensor cannot be a graph input
    assert all(torch.equal(v, before[k]) for k, v in model._flat_params().items())


# ---- 7. captured equals eager, the ids changed in place ------------------------------------------------------------------------------
KEYS = ("face_out_proj.weight", "audio_encoder_body.feat_extractor.0.conv1.weight", "audio_motion_cross_attn.layers.7.linear2.bias",
        "mask_embedding", "audio_encoder_face.feat_extractor.3.bn1.running_var", "motion_encoder.main.0.weight") + sc.TABLES


def test_captured_step_reads_the_id_buffer(golden_dir):
    """Two replays with the ids changed IN PLACE between them against two eager steps of a twin (fp32, the bars of
    test_captured_training_step_equals_the_eager_step): the graph reads the caller's buffer, not a copy of it."""
    g = sc.golden(golden_dir)
    batch, masks, random_mask, _ids = _step_inputs(g)
    model_e, vq = sc.product_models(int(g["speaker_dims"]), precision="fp32", device=DEV)
    model_g, _ = sc.product_models(int(g["speaker_dims"]), precision="fp32", device=DEV)
    eager, graphed = training.Trainer(model_e, vq), training.Trainer(model_g, vq)
    buf = torch.tensor([[2], [0], [2], [1]], dtype=torch.int64, device=DEV)
    graphed.capture(batch, random_mask, masks, speaker_id=buf)
    after_first = {}
    for step, ids in ((1, [2, 0, 2, 1]), (2, [1, 1, 3, 0])):
        buf.copy_(torch.tensor(ids, dtype=torch.int64).reshape(-1, 1))
        le = eager.step(batch, 0, masks, random_mask, speaker_id=torch.tensor(ids))
        lg = graphed.replay()
        for k in le:
            assert abs(le[k] - lg[k]) <= 1e-6 * max(1.0, abs(le[k])), (step, k, le[k], lg[k])
        pe, pg = model_e._flat_params(), model_g._flat_params()
        for k in KEYS:
            assert float((pe[k] - pg[k]).abs().max()) <= 1e-7 * max(1.0, float(pe[k].abs().max())), (step, k)
        if step == 1:
            after_first = {n: pg[n].clone() for n in sc.TABLES}
            assert all(torch.equal(pg[n][3], synthetic_row(model_g, n, 3)) for n in sc.TABLES)      # row 3: no clip named it in step 1
        else:
            assert all(not torch.equal(pg[n][3], after_first[n][3]) for n in sc.TABLES)              # ... and a clip does in step 2
    assert eager.state["face_out_proj.weight"]["step"] == 2 and graphed.state["face_out_proj.weight"]["step"] == 2


def synthetic_row(model, name, row):
    state = sc._CACHE[("state", model.config.speaker_dims, 0)]
    return state[name][row].to(DEV)


# ---- 8. the loader on the device -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drop_last", [True, False])
@pytest.mark.parametrize("world", [1, 2])
def test_loader_speaker_ids_on_the_device(world, drop_last):
    store = sc.speaker_store(DEV)
    for rank in range(world):
        loader = data.ClipLoader(store, 2, rank=rank, world=world, drop_last=drop_last, hold_iteration=not drop_last, speaker_dims=3)
        addr = loader.speaker_id.data_ptr()
        for epoch in (0, 1):
            loader.set_epoch(epoch)
            ids = data.epoch_order(store.n_clips, epoch, rank, world, 0)
            if len(ids) % 2 and not drop_last:
                ids = np.concatenate([ids, ids[:1]])
            n_batches = len(ids) // 2
            assert len(loader) == n_batches
            for k in range(n_batches + 1):                           # one past the end: the cursor wraps
                loader.fill()
                clips = ids[(k % n_batches) * 2:(k % n_batches) * 2 + 2]
                want = [int(store.speakers_host[store.clip_list[int(c)][0]]) for c in clips]
                assert loader.speaker_id.reshape(-1).tolist() == want, (world, rank, epoch, k)
                ref = store.gather_host(clips)
                assert torch.equal(loader.batch["motion"].cpu(), ref["motion"])      # the ids belong to the clips of THIS fill
                assert loader.speaker_id.data_ptr() == addr
        loader.check()
    plain = data.ClipLoader(sc.speaker_store(DEV, speakers=(0, None, 0)), 2)
    plain.fill()
    assert not plain.speaker_id.any()
    bad = data.ClipLoader(store, 2)
    bad.order[1] = 99                                                # an id outside the clip table: row zeroed, status word set
    bad.fill()
    assert int(bad.speaker_id[1]) == 0
    with pytest.raises(RuntimeError, match="status"):
        bad.check()


def test_captured_step_fed_by_the_loader_equals_the_eager_step():
    """`capture(loader.batch, loader.random_mask, prologue=loader.fill, speaker_id=loader.speaker_id)`: one replay = next batch with its ids,
    then the step; against an eager step of a twin on a copy of the same batch, mask and ids (device-drawn dropout masks, same seed)."""
    spf = data.samples_per_frame(16000)
    rng = np.random.default_rng(9)
    recs = []
    for f, s in ((70, 2), (66, 0), (68, 1)):
        recs.append(dict(poses=0.3 * rng.standard_normal((f, 165)).astype(np.float32), expressions=0.5 * rng.standard_normal((f, 100)).astype(np.float32),
                         trans=0.1 * rng.standard_normal((f, 3)).astype(np.float32), foot_contact=(rng.random((f, 4)) > 0.5).astype(np.float32),
                         audio=(0.1 * rng.standard_normal(f * spf)).astype(np.float32), speaker=s))
    store = data.ClipStore.from_arrays(recs, [(0, 0, 64), (1, 2, 66), (2, 3, 67), (0, 6, 70)], DEV)
    model_e, vq = sc.product_models(3, precision="fp32", device=DEV)
    model_g, _ = sc.product_models(3, precision="fp32", device=DEV)
    loader = data.ClipLoader(store, 2, speaker_dims=3, mask_ratio=(0.0, 0.5))
    graphed = training.Trainer(model_g, vq, seed=5).capture(loader.batch, loader.random_mask, prologue=loader.fill, speaker_id=loader.speaker_id)
    eager = training.Trainer(model_e, vq, seed=5)
    seen = set()
    for step in range(2):
        lg = graphed.replay()
        ids = loader.speaker_id.clone()
        clips = data.epoch_order(store.n_clips, 0)[2 * step:2 * step + 2]
        assert ids.reshape(-1).tolist() == [int(store.speakers_host[store.clip_list[int(c)][0]]) for c in clips]
        seen.update(ids.reshape(-1).tolist())
        le = eager.step({k: v.clone() for k, v in loader.batch.items()}, random_mask=loader.random_mask.clone(), speaker_id=ids)
        for k in le:
            assert abs(le[k] - lg[k]) <= 1e-6 * max(1.0, abs(le[k])), (step, k, le[k], lg[k])
        pe, pg = model_e._flat_params(), model_g._flat_params()
        for k in KEYS:
            assert float((pe[k] - pg[k]).abs().max()) <= 1e-7 * max(1.0, float(pe[k].abs().max())), (step, k)
    assert seen == {0, 1, 2}
    loader.check()


# ---- 9. validation -------------------------------------------------------------------------------------------------------------------
def test_validator_with_speaker_ids():
    """ids [1, 0], speaker_dims = 3: `step` and `replay` agree bit for bit, both differ from the all-zero run, and both equal the oracle's
    three eval forwards with those ids — losses within test_validation_gpu.py's step bound, codes identical outside rows whose top-2 logit
    margin is below 1e-3 (the rule of tests/golden/make_golden_val.py)."""
    from oracle import emage_train_oracle as tro
    bs, t = 2, 64
    host = common.train_batch(bs=bs)
    batch = {k: v.to(DEV) for k, v in host.items()}
    mask = (torch.rand(bs, t, 337, generator=torch.Generator().manual_seed(4)) < 0.5).float()
    ids = torch.tensor([[1], [0]], dtype=torch.int64)
    model, vq = sc.product_models(3, precision="f16x3", device=DEV)
    val = validation.Validator(model, vq)
    zero = val.step(batch, mask.to(DEV))
    got = val.step(batch, mask.to(DEV), speaker_id=ids)
    eager_codes = {tag: {p: v.clone() for p, v in d.items()} for tag, d in val.codes.items()}
    assert all(got[k] != zero[k] for k in validation.LOSS_KEYS)
    assert val.step(batch, mask.to(DEV), speaker_id=torch.zeros(bs, 1, dtype=torch.int64)) == zero
    with pytest.raises(ValueError, match="speaker_dims"):
        val.step(batch, mask.to(DEV), speaker_id=torch.tensor([3, 0]))
    buf = ids.to(DEV)
    val.capture(batch, mask.to(DEV), speaker_id=buf)
    val.reset()
    val.replay()
    r = ops.val_read(val.acc)
    assert r["last"] == [got[k] for k in validation.LOSS_KEYS]
    assert all(torch.equal(val.codes[tag][p], eager_codes[tag][p]) for tag in validation.TAGS for p in validation.PARTS)
    buf.zero_()                                                      # the graph reads the buffer
    val.replay()
    assert ops.val_read(val.acc)["last"] == [zero[k] for k in validation.LOSS_KEYS]

    omodel, (_om, ovq) = sc.oracle_audio_model(3), common.oracle_models()
    with torch.no_grad():
        index, latent, masked_motion = tro.targets(ovq, host["motion"], host["expressions"], host["trans"], host["foot_contact"])
        seed_mask = torch.ones_like(masked_motion)
        seed_mask[:, :model.config.seed_frames] = 0
        want, n_small, n_rows = {}, 0, 0
        for tag, m, use_audio in (("seed", seed_mask, True), ("audio", mask, True), ("mask", mask, False)):
            out = omodel.forward(host["audio"], ids, masked_motion, m, use_audio=use_audio)
            want["rec_" + tag], want["cls_" + tag] = float(tro.rec_loss(out, latent, model.config)), float(tro.cls_loss(out, index, model.config))
            for p in validation.PARTS:
                logits = out[f"cls_{p}"]
                top2 = torch.topk(logits, 2, dim=2)[0]
                small = (top2[..., 0] - top2[..., 1]) < 1e-3
                code = torch.log_softmax(logits, dim=2).argmax(dim=2)
                mine = eager_codes[tag][p].cpu()
                assert torch.equal(mine[~small], code[~small]), (tag, p, int((mine != code).sum()))
                n_small, n_rows = n_small + int(small.sum()), n_rows + small.numel()
    assert n_small <= 0.01 * n_rows
    want["all"] = sum(want.values())
    for k in validation.LOSS_KEYS:
        print(f"{k}: validator {got[k]:.6f}  oracle {want[k]:.6f}")
        assert np.isfinite(got[k]) and abs(got[k] - want[k]) < 2e-4 * max(1.0, abs(want[k])), (k, got[k], want[k])


# ---- 10. whole recordings --------------------------------------------------------------------------------------------------------------
FRAMES = (70, 130, 70, 64, 40)
IDS, OTHER = (2, 0, 1, 0, 2), (1, 1, 0, 2, 0)


def _copy(results):
    return [tuple(a.copy() for a in r) for r in results]


def _equal(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for ra, rb in zip(a, b) for x, y in zip(ra, rb))


def test_runner_with_per_recording_ids_equals_the_single_recording_runs():
    """Five recordings, max_batch = 2, ids [2, 0, 1, 0, 2], ONE captured pass: every recording's codes are those of `infer_codes` at B = 1
    with its own id and its arrays those of the B = 1 runner (max |diff| 0.0); a replay after `load()` of a set with other ids gives the
    other set's B = 1 results without a new graph; with equal ids the results are those of a runner built with the plain integer."""
    model, vq = sc.product_models(3, precision="f16x3", device=DEV)
    waves = [synthetic.synthetic_audio(1, synthetic.samples_for_frames(f), seed=77 + k)[0] for k, f in enumerate(FRAMES)]
    rs = R.RecordingSet.from_audio(waves, DEV, speaker_ids=IDS)
    runner = R.RecordingRunner.for_set(model, vq, rs, use_graph=True, max_batch=2)
    assert runner.per_recording_ids and runner.graph is not None
    assert any(u.lo > 0 for u in runner.units) and any(g.n > 1 for g in runner.tails)
    graph = runner.graph
    first = _copy(runner(rs))
    first_codes = [{p: v.clone() for p, v in runner.codes_of(k).items()} for k in range(len(FRAMES))]
    second = _copy(runner(R.RecordingSet.from_audio(waves, DEV, speaker_ids=OTHER)))
    second_codes = [{p: v.clone() for p, v in runner.codes_of(k).items()} for k in range(len(FRAMES))]
    assert runner.graph is graph and not _equal(first, second)
    singles = {}
    zero_trans = torch.zeros(1, 3, device=DEV)
    for k, wave in enumerate(waves):
        for ids, res, codes in ((IDS, first, first_codes), (OTHER, second, second_codes)):
            key = (k, ids[k])
            if key not in singles:                                   # the recording alone: B = 1 `infer_codes` with its id, then the B = 1 decode
                lone = model.infer_codes(wave[None].to(DEV), torch.tensor([[ids[k]]], device=DEV), vq)
                pred = vq.decode(**lone, get_global_motion=True, ref_trans=zero_trans)
                singles[key] = (tuple(pred[nm][0].cpu().numpy() for nm in ("motion_axis_angle", "expression", "trans")),
                                {p: lone[f"{p}_index"][0].clone() for p in codes[k]})
            want, want_codes = singles[key]
            for p, v in codes[k].items():
                assert torch.equal(v, want_codes[p]), (k, ids[k], p)
            for nm, a, b in zip(("poses", "expressions", "trans"), res[k], want):
                assert a.shape == b.shape and float(np.abs(a - b).max()) == 0.0, (k, ids[k], nm)
    assert not _equal([singles[(0, 2)][0]], [singles[(0, 1)][0]])      # the id matters
    same = _copy(runner(R.RecordingSet.from_audio(waves, DEV, speaker_ids=[1] * 5)))
    plain = R.RecordingRunner(model, vq, rs.sample_counts, use_graph=False, max_batch=2, speaker_id=1)
    assert not plain.per_recording_ids
    assert _equal(same, _copy(plain(R.RecordingSet.from_audio(waves, DEV))))
    with pytest.raises(ValueError, match="equal speaker ids"):
        plain.load(rs)
