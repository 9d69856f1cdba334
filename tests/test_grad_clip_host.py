"""The gradient-norm / clipping feature without a GPU: the case table of tests/grad_clip_cases.py through the CPU stand-ins of
tests/fake_grad_clip.py (a correct implementation passes every derived tolerance), the trainers' defaults (nothing new is launched or
returned), and the semantics at world size 2 on gloo: the reported norm is that of the AVERAGED gradient, the same on every rank."""
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import common
import fake_grad_clip
import fake_ops as F
import grad_clip_cases as gc
import train_common as tc
from pantomatrix_amd import training


@pytest.mark.parametrize("pre_scale,max_norm", gc.NORM_CASES)
def test_big_table(pre_scale, max_norm):
    gc.check_big_table(F, pre_scale, max_norm)


def test_zero_table():
    gc.check_zero_table(F)


@pytest.mark.parametrize("n", [1, gc.CHUNK + 1])
def test_one_tensor(n):
    gc.check_one_tensor(F, n)


@pytest.mark.parametrize("bad", [math.nan, math.inf])
def test_nonfinite(bad):
    gc.check_nonfinite(F, bad)


@pytest.mark.parametrize("start,wd", gc.ADAM_STATES)
@pytest.mark.parametrize("grad_scale", gc.GRAD_SCALES)
@pytest.mark.parametrize("coef", gc.COEFS)
def test_adam_scaled(coef, grad_scale, start, wd):
    gc.check_adam_scaled(F, coef, grad_scale, start, wd)


def test_adam_scaled_skip():
    gc.check_adam_scaled_skip(F)


def test_scale_multi():
    gc.check_scale_multi(F)


def test_max_grad_norm_is_validated_and_a_change_asks_for_a_recapture():
    model, vq = common.product_models(precision="fp32")
    with pytest.raises(ValueError):
        training.Trainer(model, vq, max_grad_norm=0.0)
    trainer = training.Trainer(model, vq, max_grad_norm=0.99)
    trainer.max_grad_norm = 0.5                       # nothing captured: nothing to re-capture
    assert trainer.max_grad_norm == 0.5 and not trainer._recapture_pending
    trainer._graph = object()                         # a captured step carries max_norm as a launch argument
    trainer.max_grad_norm = 0.5
    assert not trainer._recapture_pending
    trainer.max_grad_norm = 0.25
    assert trainer._recapture_pending
    with pytest.raises(RuntimeError):
        training.Trainer(model, vq).param_grad_norms()


def test_defaults_launch_nothing_new_and_return_no_grad_norm():
    """With the default arguments the step is the step it was: the stand-ins of tests/fake_ops.py ALONE carry it (no new op is reached, Adam
    is called without the new keyword), and the loss dict has no "grad_norm".  With the options set, the same step launches the norm once,
    hands Adam the device coefficient, and reports the norm of the hooked gradient."""
    batch, _, masks, random_mask, _ = tc.oracle_step(seed=20, iteration=0)
    model, vq = common.product_models(precision="fp32")
    seen = {}
    with F.installed(), torch.no_grad():
        losses = training.Trainer(model, vq).step(batch, 0, masks, random_mask, grad_hook=lambda g: seen.update({k: v.clone() for k, v in g.items()}))
        calls = list(F.CALLS)
    assert "grad_norm" not in losses and not set(calls) & set(fake_grad_clip.NEW_CALLS) and "adam_multi" in calls
    model2, _ = common.product_models(precision="fp32")
    want = math.sqrt(math.fsum(float((v.double() ** 2).sum()) for v in seen.values()))
    trainer = training.Trainer(model2, vq, max_grad_norm=0.5 * want)
    with fake_grad_clip.installed(), torch.no_grad():
        clipped = trainer.step(batch, 0, masks, random_mask)
        calls = list(F.CALLS)
    assert calls.count("grad_norm") == 1 and calls.count("adam_multi_scaled") == 1 and "adam_multi" not in calls and "scale_multi" not in calls
    assert calls.index("grad_norm") < calls.index("adam_multi_scaled") and max(i for i, c in enumerate(calls) if c == "count_nonfinite") < calls.index("adam_multi_scaled")
    assert {k: v for k, v in clipped.items() if k != "grad_norm"} == losses
    assert abs(clipped["grad_norm"] - want) <= gc.ulp32(want)
    coef = float(trainer._grad_norm.coef)
    assert abs(coef - 0.5 * want / (want + 1e-6)) <= gc.ulp32(0.5)
    norms = trainer.param_grad_norms()
    assert list(norms) == list(trainer.buckets.grads) and set(norms) == set(seen)
    for k in ("face_out_proj.weight", "mask_embedding", "audio_encoder_body.feat_extractor.5.conv2.weight"):
        assert abs(norms[k] - float(seen[k].double().norm())) <= 1e-12 * float(seen[k].double().norm()), k
        m = trainer.state[k]["exp_avg"]                 # Adam's first step from zero moments: exp_avg = (1 - beta1) g coef
        ref = 0.1 * seen[k].double() * coef
        assert float((m.double() - ref).abs().max()) <= 4 * 2.0 ** -24 * float(ref.abs().max()), k


def test_a_skipped_step_reports_its_nonfinite_norm():
    """An inf among the (hooked) gradients: the health word skips the update as before, and the loss dict carries the inf norm."""
    batch, _, masks, random_mask, _ = tc.oracle_step(seed=20, iteration=0)
    model, vq = common.product_models(precision="fp32")
    before = model._flat_params()["mask_embedding"].clone()
    trainer = training.Trainer(model, vq, on_nonfinite="skip", max_grad_norm=0.99)

    def poison(grads):
        grads["mask_embedding"].reshape(-1)[0] = math.inf

    with fake_grad_clip.installed(), torch.no_grad():
        losses = trainer.step(batch, 0, masks, random_mask, grad_hook=poison)
    assert losses["grad_norm"] == math.inf and trainer.skipped_steps == 1 and trainer.steps_done == 0
    assert torch.equal(model._flat_params()["mask_embedding"], before)
    assert trainer.param_grad_norms()["mask_embedding"] == math.inf and math.isfinite(trainer.param_grad_norms()["face_out_proj.weight"])
    assert float(trainer.buckets.grads["mask_embedding"].abs().max()) == 0.0        # cleared for the next step


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _norm_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import common
    import fake_grad_clip
    import train_common as tc
    from pantomatrix_amd import dist as pd
    from pantomatrix_amd import training
    assert pd.init("gloo") is not None
    torch.set_num_threads(2)
    batch, _, masks, random_mask, _ = tc.oracle_step(seed=20 + rank, iteration=0)          # each rank: its own draws (its own shard of the data)
    model, vq = common.product_models(precision="fp32")
    trainer = training.Trainer(model, vq, track_grad_norm=True)
    seen = {}
    with fake_grad_clip.installed(), torch.no_grad():
        losses = trainer.step(batch, 0, masks, random_mask, grad_hook=lambda g: seen.update(sumsq=math.fsum(float((v.double() ** 2).sum()) for v in g.values())))
    q.put((rank, losses["grad_norm"], seen["sumsq"], losses["all"]))
    pd.finalize()


def test_two_gloo_ranks_report_the_norm_of_the_averaged_gradient():
    """Two ranks with different batches: the hook sees the exchanged SUM of the gradients; both ranks report the same "grad_norm", and it is
    the float64 norm of sum / 2 — what DistributedDataParallel followed by clip_grad_norm_ sees."""
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_norm_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=1200) for _ in range(world)), key=lambda r: r[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    (_, n0, s0, l0), (_, n1, s1, l1) = res
    assert l0 != l1                                   # different data on the two ranks
    assert n0 == n1 and s0 == s1
    want = 0.5 * math.sqrt(s0)
    print(f"two ranks: grad_norm {n0!r}, float64 norm of the averaged gradient {want!r}")
    assert abs(n0 - want) <= gc.ulp32(want)
