"""The validation pass without a device: `validation.Validator` over the CPU restatement of its kernel (tests/fake_val_ops.py) against the REAL
reference's validation step (tests/golden/val_step.npz), the meter arithmetic of a pass with a short last batch, and the evaluation form of
`data.ClipLoader` (drop_last=False, hold_iteration=True) over the stand-ins of its kernels."""
import os

import numpy as np
import pytest
import torch

import clip_store_common as cc
import common
import fake_clip_ops
import fake_ops
import fake_val_ops
import val_cases as vc
from pantomatrix_amd import _lib, data, ops, validation

LOSS_KEYS = validation.LOSS_KEYS


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "val_step.npz"))


def golden_mask(g, t=64):
    n = int(g["bs"]) * t * 337
    return torch.from_numpy(np.unpackbits(g["random_mask"])[:n].astype(np.float32)).view(int(g["bs"]), t, 337)


def test_contract_restatement_equals_its_float64_form():
    """The torch restatement the host tests run on against the float64 numpy form the GPU tests use as their oracle: sums within the kernel
    bound, hit counts and row counts equal, for a full, a short and an empty batch."""
    for n_valid in (vc.CLIPS, 25, 1, 0):
        entries, frames = vc.build("cpu", n_valid=n_valid)
        acc_frame, acc = vc.framed_acc("cpu")
        with fake_val_ops.installed():
            ops.val_metrics(entries, vc.T, torch.tensor([n_valid], dtype=torch.int32), acc)
        want = fake_val_ops.val_metrics_reference(entries, vc.T, n_valid)
        got = ops.val_read(acc)
        vc.assert_frames_intact(frames, acc_frame)
        if n_valid == 0:
            assert got["batches"] == 0 and got["rows"] == 0 and got["meter"] == [0.0] * 7 and got["hits"] == [0] * 12
            continue
        assert got["batches"] == 1 and got["rows"] == want["rows"] == n_valid * vc.T and got["status"] == 0
        assert got["hits"][:3] == want["hits"] == got["last_hits"][:3]
        for k in range(7):
            assert np.isfinite(got["last"][k]) and abs(got["last"][k] - want["last"][k]) <= vc.SUM_RTOL * abs(want["last"][k]), (n_valid, k)


def test_validator_reproduces_the_reference_step(gold):
    """Three clips of `common.train_batch` through the product's eval forward (fp32 precision over the CPU stand-ins of its kernels), the
    shared WavEncoder pass and the restated `val_metrics`: the seven losses of the reference's train_val_fn(mode="val")."""
    bs = int(gold["bs"])
    batch, mask = common.train_batch(bs=bs), golden_mask(gold)
    with fake_val_ops.installed():
        model, vq = common.product_models(precision="fp32")
        val = validation.Validator(model, vq)
        before = {k: v.clone() for k, v in model.state_dict().items()}
        got = val.step(batch, mask)
        assert fake_ops.CALLS.count("val_metrics") == 1 and "mse_loss" not in fake_ops.CALLS and "nll_loss" not in fake_ops.CALLS
        assert fake_ops.CALLS.count("argmax_logsoftmax") == 0
        assert fake_ops.CALLS.count("wav_conv_in") + fake_ops.CALLS.count("wav_block0") <= 2, "the WavEncoders run once for the three forwards"
        res = val.result()
    for k, want in zip(LOSS_KEYS, gold[f"losses_b{bs}"]):
        print(f"{k}: validator {got[k]:.6f}  reference {want:.6f}")
        assert abs(got[k] - want) < vc.STEP_RTOL * max(1.0, abs(want)), k
        assert res[k] == got[k]
    assert res["batches"] == 1 and res["clips"] == bs
    assert not model.training and all(torch.equal(v, before[k]) for k, v in model.state_dict().items())
    assert val.decoded.shape == val.target_rot6d.shape == (bs, 64, 330)
    hits = dict(zip([f"{t}_{p}" for t in validation.TAGS for p in validation.PARTS], gold[f"hits_b{bs}"]))
    for t in validation.TAGS:
        for p in validation.PARTS:
            small = int(np.unpackbits(gold[f"small_b{bs}_{t}_{p}"])[:bs * 64].sum())
            assert abs(got[f"acc_{t}_{p}"] * bs * 64 - hits[f"{t}_{p}"]) <= small, (t, p)


def test_meter_over_a_pass_with_a_short_last_batch():
    """The reference's meter: every batch weighs the same, a short last one included (sum of the per-batch values / batches); accuracies are
    hits / rows over the real clips; the padding clip of the short batch — other, finite data here: the stand-in of the contraction kernel
    refuses NaN operands; the GPU tests pad with NaN — leaves no trace beyond fp32 rounding of another batch shape (a forward is ~30
    contractions of length <= 3072 deep: 2e-5), and at most one flipped arg-max."""
    t = 8
    full = common.train_batch(bs=3, t=t)
    first = {k: v[:2].clone() for k, v in full.items()}
    short = {k: torch.cat([v[2:3], v[:1] * -2.5 + 1.0]) for k, v in full.items()}
    alone = {k: v[2:3].clone() for k, v in full.items()}
    mask = (torch.rand(3, t, 337, generator=torch.Generator().manual_seed(2)) < 0.3).float()
    with fake_val_ops.installed():
        model, vq = common.product_models(precision="fp32")
        val = validation.Validator(model, vq)
        a = val.step(first, mask[:2])
        b = val.step(short, torch.cat([mask[2:3], mask[:1]]), n_valid=1)
        res = val.result()
        val.reset()
        c = val.step(alone, mask[2:3])
        assert val.result()["batches"] == 1
    assert res["batches"] == 2 and res["clips"] == 3
    for k in LOSS_KEYS:
        assert np.isfinite(b[k]) and abs(b[k] - c[k]) <= 2e-5 * max(1.0, abs(c[k])), k
        assert abs(res[k] - (a[k] + b[k]) / 2) <= 1e-12 * max(1.0, abs(res[k])), k
    for tag in validation.TAGS:
        for p in validation.PARTS:
            k = f"acc_{tag}_{p}"
            assert abs(b[k] - c[k]) * t <= 1 + 1e-9 and abs(res[k] - (a[k] * 2 * t + b[k] * t) / (3 * t)) < 1e-12, k


def test_argument_validation_without_gpu():
    """Every refusal happens before the launch, so it can be exercised here (the pointers are never dereferenced)."""
    lib = _lib.load()
    for what, args in vc.refused_calls():
        assert lib.emage_val_metrics(*args) == -1, what
    assert lib.emage_val_metrics_workspace_bytes(0, 3) == -1 and lib.emage_val_metrics_workspace_bytes(vc.M, 13) == -1
    assert lib.emage_val_metrics_workspace_bytes(vc.M, 3) == 3 * 9 * 32


def test_status_word_raises_and_reset_clears_it():
    entries, _frames = vc.build("cpu", bad_index=True)
    with fake_val_ops.installed():
        acc = ops.val_accumulators("cpu")
        ops.val_metrics(entries, vc.T, torch.tensor([vc.CLIPS], dtype=torch.int32), acc)
        assert ops.val_read(acc)["status"] == 1
        model, vq = common.product_models(precision="fp32")
        val = validation.Validator(model, vq)
        val.acc.copy_(acc)
        val._frames = vc.T
        with pytest.raises(_lib.EmageKernelError, match="out of range"):
            val.result()
        val.reset()
        with pytest.raises(RuntimeError, match="no batch"):
            val.result()


# ---- the evaluation loader ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def store():
    recordings, clips = cc.make_recordings()
    return data.ClipStore.from_arrays(recordings, clips, "cpu")


@pytest.mark.parametrize("world,rank", [(1, 0), (2, 1)])
def test_evaluation_loader_counts_the_short_last_batch(store, world, rank):
    batch = 3
    ids = data.epoch_order(store.n_clips, 0, rank, world)
    n_batches = -(-len(ids) // batch)
    with fake_clip_ops.installed():
        loader = data.ClipLoader(store, batch, rank=rank, world=world, drop_last=False, hold_iteration=True)
        assert len(loader) == n_batches and loader.order.numel() == n_batches * batch
        order = loader.order.tolist()
        assert order[:len(ids)] == ids.tolist() and all(0 <= i < store.n_clips for i in order[len(ids):])
        loader.iteration = 40
        for i in range(n_batches + 1):                       # one past the end: the cursor wraps to the first batch
            loader.fill()
            real = min(batch, len(ids) - (i % n_batches) * batch)
            assert int(loader.valid) == real and loader.valid.dtype == torch.int32
            want = store.gather_host(ids[(i % n_batches) * batch:(i % n_batches) * batch + real])
            for k in cc.KEYS:
                assert torch.equal(loader.batch[k][:real], want[k]), (i, k)
            assert int(loader.cursor) == i + 1 and loader.iteration == 40
            assert torch.equal(loader.random_mask.reshape(-1), torch.from_numpy(ops.motion_mask_reference(loader.random_mask.numel(), loader.mask_a,
                                                                                                           loader.mask_b, 0, data.MOTION_MASK_ID, 40)))
        loader.check()
        assert loader.prologue_state()[0] is loader.counters and any(t is loader.valid for t in loader.prologue_state())


def test_default_loader_is_unchanged(store, golden_dir):
    """drop_last=True, hold_iteration=False (the defaults): the batches of tests/golden/clip_store.npz, `valid` constant, no extra launch."""
    gold = cc.golden(golden_dir)
    world, rank = cc.RANKS[1]
    with fake_clip_ops.installed():
        loader = data.ClipLoader(store, cc.BATCH, rank=rank, world=world)
        assert loader.drop_last and not loader.hold_iteration and len(loader.prologue_state()) == 1
        for epoch in cc.EPOCHS:
            loader.set_epoch(epoch)
            order, batches = cc.golden_batches(gold, world, rank, epoch)
            assert len(loader) == len(batches) == len(order) // cc.BATCH
            for i, want in enumerate(batches):
                loader.fill()
                cc.assert_batches_equal(loader.batch, want, (epoch, i))
                assert int(loader.valid) == cc.BATCH
        assert loader.iteration == len(cc.EPOCHS) * len(loader)
        assert fake_ops.CALLS.count("gather_clips") == fake_ops.CALLS.count("motion_mask") == loader.iteration
