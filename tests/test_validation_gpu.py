"""The validation pass on the MI355X: `emage_val_metrics` against the float64 restatement of its contract (tests/fake_val_ops.py) on the
cases of tests/val_cases.py — inputs are views inside larger tensors whose slack holds valid data, outputs sit inside canary frames: a missing
guard shows as a wrong number, never as an access outside an allocation —, and `validation.Validator` against the REAL reference's validation
step (tests/golden/val_step.npz), as a captured graph, beside a `Trainer`, and fed by the evaluation loader."""
import os

import numpy as np
import pytest
import torch

import common
import fake_val_ops
import val_cases as vc
from pantomatrix_amd import _lib, data, ops, training, validation

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOSS_KEYS = validation.LOSS_KEYS


def i32(v):
    return torch.tensor([v], dtype=torch.int32, device=DEV)


def within_step_bound(got, want, what):
    assert np.isfinite(got) and abs(got - want) < vc.STEP_RTOL * max(1.0, abs(want)), (what, got, want)


# ---- the kernel -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_valid", [26, 25, 1, 0])
def test_kernel_against_float64(n_valid):
    """Sums within 1e-5 relative of float64 log-softmax / NLL / MSE over the valid prefix (rows beyond it are NaN) and finite; pred_index
    bit-equal to `ops.argmax_logsoftmax` on the same logits for EVERY row — the duplicated maximum, the all-NaN rows and the row with one NaN
    included; hit counts exact; n_valid = 0 leaves the meter, the counters and `batches` as an earlier call left them."""
    entries, frames = vc.build(DEV, n_valid=n_valid)
    acc_frame, acc = vc.framed_acc(DEV)
    before = None
    if n_valid == 0:                                         # something to leave untouched
        earlier, _f = vc.build(DEV, n_valid=vc.CLIPS, seed=3)
        ops.val_metrics(earlier, vc.T, i32(vc.CLIPS), acc)
        before = acc.clone()
    ws = ops.val_metrics(entries, vc.T, i32(n_valid), acc)
    torch.cuda.synchronize()
    vc.assert_frames_intact(frames, acc_frame)
    for e in entries:
        assert torch.equal(e["pred"], ops.argmax_logsoftmax(e["logits"])), "arg-max differs from emage_argmax_logsoftmax_f32"
    if n_valid == 0:                                         # every row is poisoned: only the arg-max rule and the untouched block are left to check
        assert torch.equal(acc.view(torch.int64), before.view(torch.int64))
        return
    assert int(entries[0]["pred"][3]) == 10                  # the first of the two equal maxima
    got, want = ops.val_read(acc), fake_val_ops.val_metrics_reference(entries, vc.T, n_valid)
    assert got["batches"] == 1 and got["rows"] == got["last_rows"] == n_valid * vc.T and got["status"] == 0
    assert got["hits"][:3] == want["hits"] == got["last_hits"][:3] and got["hits"][3:] == [0] * 9
    for k in range(7):
        print(f"n_valid {n_valid} last[{k}]: kernel {got['last'][k]:.9f}  float64 {want['last'][k]:.9f}")
        assert np.isfinite(got["last"][k]) and abs(got["last"][k] - want["last"][k]) <= vc.SUM_RTOL * abs(want["last"][k]), k
        assert got["meter"][k] == got["last"][k]
    assert ws.numel() * 8 >= _lib.load().emage_val_metrics_workspace_bytes(vc.M, 3)


def test_kernel_accumulates_in_a_fixed_order():
    """Two calls on different data: the meter is the sum of the two per-batch values, hits and rows add up, batches == 2; the same
    sequence again gives the same bits in every word of the accumulator block."""
    blocks = []
    for _run in range(2):
        _frame, acc = vc.framed_acc(DEV)
        lasts, hits, ws = [], [], None
        for seed, n_valid in ((0, 26), (1, 25)):
            entries, _f = vc.build(DEV, n_valid=n_valid, seed=seed)
            ws = ops.val_metrics(entries, vc.T, i32(n_valid), acc, ws)
            r = ops.val_read(acc)
            lasts.append(r["last"])
            hits.append(r["last_hits"])
        assert r["batches"] == 2 and r["rows"] == (26 + 25) * vc.T
        for k in range(7):
            assert r["meter"][k] == lasts[0][k] + lasts[1][k]
        assert r["hits"] == [a + b for a, b in zip(*hits)]
        blocks.append(acc.clone())
    assert torch.equal(blocks[0].view(torch.int64), blocks[1].view(torch.int64))


def test_kernel_reports_an_index_outside_the_codebook():
    clean, _f = vc.build(DEV)
    entries, _f = vc.build(DEV, bad_index=True)
    _frame, acc = vc.framed_acc(DEV)
    _frame2, acc_clean = vc.framed_acc(DEV)
    ops.val_metrics(entries, vc.T, i32(vc.CLIPS), acc)
    ops.val_metrics(clean, vc.T, i32(vc.CLIPS), acc_clean)
    got, ref = ops.val_read(acc), ops.val_read(acc_clean)
    want = fake_val_ops.val_metrics_reference(entries, vc.T, vc.CLIPS)
    assert got["status"] == 1 and ref["status"] == 0 and want["bad"] == 1
    assert got["hits"][:3] == want["hits"] and ref["hits"][1] - got["hits"][1] in (0, 1)      # the row adds no hit
    assert abs(got["last"][3] - want["last"][3]) <= vc.SUM_RTOL * abs(want["last"][3]) and got["last"][3] < ref["last"][3]      # the row adds no NLL
    ops.val_metrics(clean, vc.T, i32(vc.CLIPS), acc)
    assert ops.val_read(acc)["status"] == 1                  # sticky


def test_argument_validation_launches_nothing():
    lib = _lib.load()
    for what, args in vc.refused_calls():
        assert lib.emage_val_metrics(*args) == -1, what
    torch.cuda.synchronize()


# ---- the step against the reference ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "val_step.npz"))


def golden_mask(g, t=64):
    n = int(g["bs"]) * t * 337
    return torch.from_numpy(np.unpackbits(g["random_mask"])[:n].astype(np.float32)).view(int(g["bs"]), t, 337)


def small_rows(g, bs, tag, part, t=64):
    return np.unpackbits(g[f"small_b{bs}_{tag}_{part}"])[:bs * t].astype(bool).reshape(bs, t)


def check_against_golden(val, got, g, bs, batch):
    """Losses within the step bound; codes equal to the golden outside its small-margin rows; hit counts equal once those rows are removed
    on both sides."""
    for k, want in zip(LOSS_KEYS, g[f"losses_b{bs}"]):
        print(f"bs {bs} {k}: validator {got[k]:.6f}  reference {want:.6f}")
        within_step_bound(got[k], float(want), k)
    index, _latent, _mm = training.targets(val.vq, *(batch[k][:bs] for k in ("motion", "expressions", "trans", "foot_contact")))
    agree = np.ones((bs, 64), dtype=bool)
    for tag in validation.TAGS:
        for p in validation.PARTS:
            small = small_rows(g, bs, tag, p)
            ref = g[f"codes_b{bs}_{tag}_{p}"].astype(np.int64)
            mine = val.codes[tag][p][:bs].cpu().numpy()
            assert np.array_equal(mine[~small], ref[~small]), (tag, p, int((mine != ref).sum()))
            gt = index[p][:bs].cpu().numpy()
            assert int((mine == gt)[~small].sum()) == int((ref == gt)[~small].sum())
            total = round(got[f"acc_{tag}_{p}"] * bs * 64)
            assert total == int((mine == gt).sum()), (tag, p)
            if tag == "seed":
                agree &= (mine == ref)
    return agree


@pytest.fixture(scope="module")
def models():
    return common.product_models(precision="f16x3", device=DEV)


def test_step_against_the_reference(gold, models):
    """3 clips, f16x3: the reference's train_val_fn(mode="val") — losses, codes, hit counts — and the decoded rot-6D of the first clip
    within 1e-3 (the tolerance of test_parity_gpu.py) on frames whose decode window (5 + vae_layer frames either side) holds only agreeing
    codes."""
    model, vq = models
    bs = int(gold["bs"])
    batch = {k: v.to(DEV) for k, v in common.train_batch(bs=bs).items()}
    val = validation.Validator(model, vq)
    got = val.step(batch, golden_mask(gold).to(DEV))
    agree = check_against_golden(val, got, gold, bs, batch)
    assert ops.val_read(val.acc)["last_rows"] == bs * 64
    reach = 5 + 2
    ok = np.array([agree[0, max(0, t - reach):t + reach + 1].all() for t in range(64)])
    assert ok.sum() >= 32, "too few comparable frames"
    err = float((val.decoded[0].cpu()[torch.from_numpy(ok)] - torch.from_numpy(gold["decoded_clip0"])[torch.from_numpy(ok)]).abs().max())
    print(f"decoded clip 0: max abs err {err:.3e} on {int(ok.sum())} frames")
    assert err < 1e-3
    assert torch.equal(val.target_rot6d, training.targets(vq, *(batch[k] for k in ("motion", "expressions", "trans", "foot_contact")))[2][:, :, :330])


def test_partial_batch_counts_only_its_real_clips(gold, models):
    """The 3-clip batch with n_valid = 2 and the third clip's audio and motion NaN: the reference's 2-clip step, accuracies over 2 x 64 rows."""
    model, vq = models
    full = {k: v.to(DEV) for k, v in common.train_batch(bs=3).items()}
    batch = {k: v.clone() for k, v in full.items()}
    batch["audio"][2] = float("nan")
    batch["motion"][2] = float("nan")
    val = validation.Validator(model, vq)
    got = val.step(batch, golden_mask(gold).to(DEV), n_valid=2)
    check_against_golden(val, got, gold, 2, full)
    r = ops.val_read(val.acc)
    assert r["last_rows"] == r["rows"] == 2 * 64 and val.result()["clips"] == 2


# ---- capture, training, the loader ----------------------------------------------------------------------------------------------------
def read_last(val):
    r = ops.val_read(val.acc)
    return r["last"] + [float(h) for h in r["last_hits"]]


@pytest.fixture(scope="module")
def scenario(gold):
    """One model validated eagerly, captured, replayed, trained for a step, replayed and validated eagerly again; a twin that only trains."""
    bs = int(gold["bs"])
    batch = {k: v.to(DEV) for k, v in common.train_batch(bs=bs).items()}
    mask = golden_mask(gold).to(DEV)
    out = {}
    model, vq = common.product_models(precision="f16x3", device=DEV)
    model.train()                                            # as inside a training loop
    before = {k: v.clone() for k, v in model.state_dict().items()}
    val = validation.Validator(model, vq)
    val.step(batch, mask)
    out["eager0"] = read_last(val)
    val.capture(batch, mask)
    val.reset()
    val.replay()
    out["replay0"] = read_last(val)
    val.replay()
    out["replay0_again"] = read_last(val)
    out["batches_after_two"] = ops.val_read(val.acc)["batches"]
    out["flag_kept"] = model.training
    out["state_kept"] = all(torch.equal(v, before[k]) for k, v in model.state_dict().items()) and list(before) == list(model.state_dict())
    trainer = training.Trainer(model, vq, seed=3)
    out["train_validated"] = trainer.step(batch, random_mask=mask)
    val.reset()
    val.replay()
    out["replay1"] = read_last(val)
    val.reset()
    val.step(batch, mask)
    out["eager1"] = read_last(val)
    twin, vq2 = common.product_models(precision="f16x3", device=DEV)
    twin.train()
    out["train_twin"] = training.Trainer(twin, vq2, seed=3).step(batch, random_mask=mask)
    return out


def test_capture_and_replay(scenario):
    """`capture` + `replay` against the eager `step` on the same inputs: BIT-EQUAL — both issue the same launches on the same operands (the
    eval forward has no atomics: its split-K adds the slices in slice order, `emage_val_metrics` its partials in block order), so the graph
    only changes who issues them.  Two replays: the same bits.  After one `Trainer.step` the replay sees the updated parameters: it differs
    from before and equals an eager step on the updated model."""
    s = scenario
    assert s["replay0"] == s["eager0"] and s["replay0_again"] == s["replay0"] and s["batches_after_two"] == 2
    assert s["replay1"] != s["replay0"] and s["replay1"][:7] != s["replay0"][:7]
    assert s["replay1"] == s["eager1"]
    assert all(np.isfinite(v) for v in s["replay1"])


def test_validation_leaves_the_model_as_found(scenario):
    """`state_dict()` and `model.training` are bit-identical across an eager and a captured validation, and the `Trainer.step` that follows
    has the loss bits of the same step on a twin model that never validated."""
    s = scenario
    assert s["flag_kept"] and s["state_kept"]
    assert s["train_validated"] == s["train_twin"], (s["train_validated"], s["train_twin"])


def test_loader_fed_epoch():
    """7 clips, batch 3, drop_last=False, hold_iteration=True, captured with the loader's fill as prologue and its `valid` as n_valid: three
    replays are an epoch of 7 clips in 3 batches whose meter means equal three eager steps on `gather_host` batches of 3, 3 and 1 clips
    (another batch shape takes other tiles: the step bound, not bits)."""
    t = 64
    rng = np.random.default_rng(4)
    f = t + 18
    rec = dict(poses=(0.3 * rng.standard_normal((f, 165))).astype(np.float32), expressions=(0.5 * rng.standard_normal((f, 100))).astype(np.float32),
               trans=(0.1 * rng.standard_normal((f, 3))).astype(np.float32), foot_contact=rng.integers(0, 2, (f, 4)).astype(np.float32),
               audio=(0.1 * rng.standard_normal(f * data.samples_per_frame(16000) + 3)).astype(np.float32))
    store = data.ClipStore.from_arrays([rec], [(0, s, s + t) for s in range(0, 19, 3)], DEV)
    assert store.n_clips == 7
    model, vq = common.product_models(precision="f16x3", device=DEV)
    loader = data.ClipLoader(store, 3, drop_last=False, hold_iteration=True, mask_seed=9)
    loader.iteration = 0
    assert len(loader) == 3
    val = validation.Validator(model, vq)
    val.capture(loader.batch, loader.random_mask, prologue=loader.fill, n_valid=loader.valid)
    assert int(loader.cursor) == 0 and loader.iteration == 0
    val.reset()
    valid = []
    for _ in range(len(loader)):
        val.replay()
        valid.append(int(loader.valid))
    res = val.result()
    loader.check()
    assert valid == [3, 3, 1] and res["clips"] == 7 and res["batches"] == 3 and loader.iteration == 0 and int(loader.cursor) == 3
    mask = torch.from_numpy(ops.motion_mask_reference(3 * t * 337, loader.mask_a, loader.mask_b, 9, data.MOTION_MASK_ID, 0)).view(3, t, 337).to(DEV)
    ids = data.epoch_order(7, 0)
    eager = validation.Validator(model, vq)
    steps = []
    for i in range(3):
        b = {k: v.to(DEV) for k, v in store.gather_host(ids[3 * i:3 * i + 3]).items()}
        steps.append(eager.step(b, mask[:b["audio"].shape[0]]))
    for k in LOSS_KEYS:
        want = sum(s[k] for s in steps) / 3
        print(f"epoch {k}: replays {res[k]:.6f}  eager steps {want:.6f}")
        within_step_bound(res[k], want, k)
    for tag in validation.TAGS:
        for p in validation.PARTS:
            assert 0.0 <= res[f"acc_{tag}_{p}"] <= 1.0
