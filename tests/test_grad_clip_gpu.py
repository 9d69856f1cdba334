"""Gradient norm and clipping inside the device training step, on the MI355X: the kernels against float64 (tests/grad_clip_cases.py),
`Trainer` / `TokenizerTrainer` with `track_grad_norm` against the gradient norms of the REAL reference's steps
(tests/golden/train_step_b2.npz, vq_train_step.npz), clipping against float64 arithmetic on the hooked gradients of an unclipped twin,
the captured step against the eager one, and the stand-alone `training.clip_grad_norm_` on the class-API loop's gradients."""
import math
import os

import numpy as np
import pytest
import torch

import common
import grad_clip_cases as gc
import train_common as tc
import vq_train_common as vc
from pantomatrix_amd import _lib, ops, training, training_vq

pytestmark = pytest.mark.gpu
DEV = "cuda"
B1, B2 = float(np.float32(0.9)), float(np.float32(0.999))       # the betas as they cross the C ABI


# ---- kernels --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pre_scale,max_norm", gc.NORM_CASES)
def test_big_table(pre_scale, max_norm):
    gc.check_big_table(ops, pre_scale, max_norm)


def test_zero_table():
    gc.check_zero_table(ops)


@pytest.mark.parametrize("n", [1, gc.CHUNK + 1])
def test_one_tensor(n):
    gc.check_one_tensor(ops, n)


@pytest.mark.parametrize("bad", [math.nan, math.inf])
def test_nonfinite(bad):
    gc.check_nonfinite(ops, bad)


@pytest.mark.parametrize("start,wd", gc.ADAM_STATES)
def test_adam_scaled(start, wd):
    for coef in gc.COEFS:
        for grad_scale in gc.GRAD_SCALES:
            gc.check_adam_scaled(ops, coef, grad_scale, start, wd)


def test_adam_scaled_skip():
    gc.check_adam_scaled_skip(ops)


def test_adam_scaled_with_a_null_factor_is_adam_multi():
    """emage_adam_multi_scaled(grad_scale_dev = NULL) through the C ABI: bit-equal to emage_adam_multi."""
    lib = _lib.load()
    _, a = gc._adam_live(10002, DEV)
    _, b = gc._adam_live(10002, DEV)
    ta, tb = (ops.AdamTable([(p, g, m, v) for p, m, v, g in x], DEV) for x in (a, b))
    hp = gc.fc.ADAM_HP
    stream = torch.cuda.current_stream().cuda_stream
    rc = lib.emage_adam_multi_scaled(ta.table.data_ptr(), ta.block_tensor.data_ptr(), ta.block_chunk.data_ptr(), ta.n_blocks, None, 10002, hp["lr"],
                                     hp["beta1"], hp["beta2"], hp["eps"], 0.01, 1.0 / 3.0, None, 1, None, stream)
    assert rc == 0
    ops.adam_multi(tb, 10002, weight_decay=0.01, grad_scale=1.0 / 3.0, zero_grad=True, **hp)
    for x, y in zip(a, b):
        for s, t in zip(x, y):
            assert gc.fc.bits_equal(s, t)


def test_scale_multi():
    gc.check_scale_multi(ops)


def test_invalid_arguments_are_refused():
    lib = _lib.load()
    assert lib.emage_grad_norm_workspace_bytes(0, 1) == 0 and lib.emage_grad_norm_workspace_bytes(3, 2) >= 3 * 8 + 2 * 4
    g = torch.ones(5, device=DEV)
    tab = ops.AdamTable([(g, g, g, g)], DEV)
    out = ops.GradNorm(tab)
    args = lambda **kw: [kw.get("table", tab.table.data_ptr()), tab.block_tensor.data_ptr(), tab.block_chunk.data_ptr(), kw.get("n_blocks", 1), kw.get("n_tensors", 1),
                         kw.get("pre_scale", 1.0), kw.get("max_norm", 1.0), out.tensor_sumsq.data_ptr(), out.total_sumsq.data_ptr(), out.norm.data_ptr(),
                         kw.get("coef", out.coef.data_ptr()), out.workspace.data_ptr(), kw.get("ws_bytes", out.workspace.numel() * 8), None]
    for bad in (dict(table=None), dict(n_blocks=0), dict(n_tensors=0), dict(pre_scale=-1.0), dict(pre_scale=math.inf), dict(max_norm=math.nan),
                dict(coef=None), dict(ws_bytes=8)):
        assert lib.emage_grad_sumsq_multi(*args(**bad)) == -1, bad
    assert lib.emage_scale_multi(tab.table.data_ptr(), tab.block_tensor.data_ptr(), tab.block_chunk.data_ptr(), 1, None, None) == -1
    assert lib.emage_scale_multi(None, tab.block_tensor.data_ptr(), tab.block_chunk.data_ptr(), 1, out.coef.data_ptr(), None) == -1
    assert lib.emage_adam_multi_scaled(None, None, None, 0, None, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, None, 0, None, None) == -1
    torch.cuda.synchronize()
    assert float(g.sum()) == 5.0


# ---- helpers --------------------------------------------------------------------------------------------------------------------------
def ulp32_of(x64):
    """Spacing of the fp32 numbers at |x| for a float64 tensor, floored at the smallest NORMAL number: results below the normal range may
    be rounded to a subnormal or flushed."""
    _m, e = torch.frexp(x64.abs())
    return torch.ldexp(torch.ones_like(x64), e - 24).clamp_(min=2.0 ** -126)


def sumsq64(grads):
    """float64 sum of squares of a dict of device gradients -> Python float (one synchronisation)."""
    return float(torch.stack([(g.double() ** 2).sum() for g in grads.values()]).sum())


def check_first_step_moments(tag, state, grads, coef):
    """Adam's first step from zero moments with the clipped gradient gc = fp32(g * coef): exp_avg = (1 - beta1) gc and
    exp_avg_sq = (1 - beta2) gc^2, elementwise within 2 fp32 ulp of the float64 values (the kernel rounds each product once: <= 1.5 ulp)."""
    c = torch.tensor(coef, dtype=torch.float32, device=DEV)
    worst = torch.zeros(2, dtype=torch.float64, device=DEV)
    for name, g in grads.items():
        gcl = (g * c).double()
        for i, (key, ref) in enumerate((("exp_avg", (1.0 - B1) * gcl), ("exp_avg_sq", (1.0 - B2) * gcl * gcl))):
            err = (state[name][key].double() - ref).abs() / ulp32_of(ref)
            worst[i] = torch.maximum(worst[i], torch.nan_to_num(err, nan=math.inf).max())
    worst = worst.tolist()
    print(f"{tag}: exp_avg within {worst[0]:.3f} ulp, exp_avg_sq within {worst[1]:.3f} ulp of the float64 values over {len(grads)} parameters")
    assert worst[0] <= 2.0 and worst[1] <= 2.0, (tag, worst)


@pytest.fixture(scope="module")
def step_inputs(golden_dir):
    g = np.load(os.path.join(golden_dir, "train_step_b2.npz"))
    batch, _, masks, random_mask, _ = tc.oracle_step(int(g["seed"]), int(g["iteration"]))
    return (g, {k: v.to(DEV) for k, v in batch.items()}, [[m.to(DEV).contiguous() for m in fm] for fm in masks], random_mask.to(DEV))


# ---- pinned to the real reference -----------------------------------------------------------------------------------------------------
def test_tracked_norms_match_the_reference_step(step_inputs):
    """`Trainer(track_grad_norm=True)` in f16x3 on the step of train_step_b2.npz: `param_grad_norms()` against the golden's 481 norms at
    the tolerances of test_training_step_matches_the_reference_..., and "grad_norm" against sqrt(sum norms^2) within what those imply:
    d N = sum n_i d n_i / N <= sum n_i (t_i n_i + 1e-6 gmax) / N."""
    g, batch, masks, random_mask = step_inputs
    model, vq = common.product_models(precision="f16x3", device=DEV)
    trainer = training.Trainer(model, vq, track_grad_norm=True)
    losses = trainer.step(batch, int(g["iteration"]), masks, random_mask)
    norms = trainer.param_grad_norms()
    gmax = float(np.max(g["grad_norms"]))
    total = math.sqrt(math.fsum(float(n) ** 2 for n in g["grad_norms"]))
    checked, bound = 0, 0.0
    for n, norm, shadowed in zip([str(x) for x in g["grad_names"]], g["grad_norms"], g["shadowed"]):
        assert n in norms, n
        if shadowed:
            continue
        tol = 3e-2 if n.startswith(("audio_encoder_face.", "audio_encoder_body.")) else 5e-3
        assert abs(norms[n] - float(norm)) <= tol * float(norm) + 1e-6 * gmax, (n, norms[n], float(norm))
        bound += float(norm) * (tol * float(norm) + 1e-6 * gmax) / total
        checked += 1
    print(f"tracked step: {checked} norms match; grad_norm {losses['grad_norm']:.4f} vs {total:.4f} (bound {bound:.3f} = {bound / total:.2e} relative)")
    assert checked > 440 and set(losses) == {"rec_seed", "cls_seed", "rec_audio", "cls_audio", "rec_mask", "cls_mask", "all", "grad_norm"}
    assert abs(losses["grad_norm"] - total) <= bound
    assert abs(losses["all"] - float(g["loss_all"])) < 2e-4 * max(1.0, abs(float(g["loss_all"])))      # "all" is still the sum of the six losses
    own = math.sqrt(math.fsum(v * v for v in norms.values()))
    assert abs(losses["grad_norm"] - own) <= gc.ulp32(own)


def test_tokenizer_tracked_norms_match_the_reference_step(golden_dir):
    g = np.load(os.path.join(golden_dir, "vq_train_step.npz"))
    m = vc.product_model("vq2", "f16x3", DEV)
    trainer = training_vq.TokenizerTrainer(m, lr=vc.LR, betas=vc.BETAS, eps=vc.EPS, track_grad_norm=True)
    res = trainer.step(vc.case_input("vq2").to(DEV))
    norms = trainer.param_grad_norms()
    names = [str(n) for n in g["vq2_grad_names"]]
    gmax = float(np.max(g["vq2_grad_norms"]))
    assert set(names) == set(norms)
    bound, total = 0.0, math.sqrt(math.fsum(float(n) ** 2 for n in g["vq2_grad_norms"]))
    for n, norm in zip(names, g["vq2_grad_norms"]):
        assert abs(norms[n] - float(norm)) <= 5e-3 * float(norm) + 1e-6 * gmax, (n, norms[n], float(norm))
        bound += float(norm) * (5e-3 * float(norm) + 1e-6 * gmax) / total
    print(f"vq2 tracked step: {len(names)} norms match; grad_norm {res['grad_norm']:.6f} vs {total:.6f}")
    assert abs(res["grad_norm"] - total) <= bound


# ---- clipping acts, and only when asked -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def unclipped(step_inputs):
    """Trainer A (no options; its gradients hooked) and its tracking twin, fp32, one step each."""
    g, batch, masks, random_mask = step_inputs
    model, vq = common.product_models(precision="fp32", device=DEV)
    a = training.Trainer(model, vq)
    grads = {}
    la = a.step(batch, 0, masks, random_mask, grad_hook=lambda gr: grads.update({k: v.clone() for k, v in gr.items()}))
    model_t, _ = common.product_models(precision="fp32", device=DEV)
    lt = training.Trainer(model_t, vq, track_grad_norm=True).step(batch, 0, masks, random_mask)
    assert "grad_norm" not in la and {k: v for k, v in lt.items() if k != "grad_norm"} == la
    return a, la, grads, lt["grad_norm"], vq


def test_a_bound_out_of_reach_changes_no_bit(step_inputs, unclipped):
    """max_grad_norm = 1e30: coef = 1.0f, and s = grad_scale * 1.0f is grad_scale — parameters and both moments bit-equal to trainer A's."""
    _g, batch, masks, random_mask = step_inputs
    a, la, _grads, _n, vq = unclipped
    model, _ = common.product_models(precision="fp32", device=DEV)
    c = training.Trainer(model, vq, max_grad_norm=1e30)
    lc = c.step(batch, 0, masks, random_mask)
    assert float(c._grad_norm.coef) == 1.0 and {k: v for k, v in lc.items() if k != "grad_norm"} == la
    pa, pc = a.fwd.model._flat_params(), model._flat_params()
    for k in pa:
        assert torch.equal(pa[k], pc[k]), k
    for k, st in a.state.items():
        assert torch.equal(st["exp_avg"], c.state[k]["exp_avg"]) and torch.equal(st["exp_avg_sq"], c.state[k]["exp_avg_sq"]), k


def test_clipping_scales_the_gradient_adam_sees(step_inputs, unclipped):
    _g, batch, masks, random_mask = step_inputs
    a, _la, grads, norm_a, vq = unclipped
    total = sumsq64(grads)
    max_norm = 0.5 * norm_a
    model, _ = common.product_models(precision="fp32", device=DEV)
    b = training.Trainer(model, vq, max_grad_norm=max_norm)
    lb = b.step(batch, 0, masks, random_mask)
    want_n, want_c = gc.formula(total, 1.0, max_norm)
    coef = float(b._grad_norm.coef)
    print(f"clipped step: grad_norm {lb['grad_norm']!r} (tracking twin {norm_a!r}, float64 {want_n!r}); coef {coef!r} (float64 {want_c!r})")
    assert lb["grad_norm"] == norm_a
    assert abs(norm_a - want_n) <= gc.ulp32(want_n) and abs(coef - want_c) <= gc.ulp32(want_c) and 0.49 < coef < 0.51
    check_first_step_moments("Trainer", b.state, grads, coef)
    assert float(torch.stack([g.abs().max() for g in b.buckets.grads.values()]).max()) == 0.0        # Adam cleared the gradients


def test_tokenizer_clipping_scales_the_gradient_adam_sees():
    x = vc.case_input("vq2").to(DEV)
    mk = lambda **kw: training_vq.TokenizerTrainer(vc.product_model("vq2", "fp32", DEV), lr=vc.LR, betas=vc.BETAS, eps=vc.EPS, **kw)
    grads = {}
    a, t = mk(), mk(track_grad_norm=True)
    la = a.step(x, grad_hook=lambda gr: grads.update({k: v.clone() for k, v in gr.items()}))
    lt = t.step(x)
    assert "grad_norm" not in la and {k: v for k, v in lt.items() if k != "grad_norm"} == la
    c = mk(max_grad_norm=1e30)
    c.step(x)
    for k in a.names:
        assert torch.equal(a.state[k]["exp_avg"], c.state[k]["exp_avg"]) and torch.equal(a.state[k]["exp_avg_sq"], c.state[k]["exp_avg_sq"]), k
        assert torch.equal(a.model._flat_params()[k], c.model._flat_params()[k]), k
    total = sumsq64(grads)
    b = mk(max_grad_norm=0.5 * lt["grad_norm"])
    lb = b.step(x)
    want_n, want_c = gc.formula(total, 1.0, 0.5 * lt["grad_norm"])
    coef = float(b._grad_norm.coef)
    assert lb["grad_norm"] == lt["grad_norm"] and abs(lb["grad_norm"] - want_n) <= gc.ulp32(want_n) and abs(coef - want_c) <= gc.ulp32(want_c)
    check_first_step_moments("TokenizerTrainer", b.state, grads, coef)


# ---- captured -------------------------------------------------------------------------------------------------------------------------
def test_captured_clipping_step_equals_the_eager_step(step_inputs):
    """A clipping trainer as ONE hipGraph (norm, coefficient and Adam's read of it inside the graph) against an eager twin: two steps,
    the criterion of test_captured_training_step_equals_the_eager_step for the parameters, equal "grad_norm" values per step."""
    _g, batch, masks, random_mask = step_inputs
    model_e, vq = common.product_models(precision="fp32", device=DEV)
    model_g, _ = common.product_models(precision="fp32", device=DEV)
    eager, graphed = training.Trainer(model_e, vq, max_grad_norm=0.99), training.Trainer(model_g, vq, max_grad_norm=0.99)
    graphed.capture(batch, random_mask, masks)
    keys = ("face_out_proj.weight", "audio_encoder_body.feat_extractor.0.conv1.weight", "audio_motion_cross_attn.layers.7.linear2.bias",
            "mask_embedding", "audio_encoder_face.feat_extractor.3.bn1.running_var", "motion_encoder.main.0.weight")
    seen = []
    for step in (1, 2):
        le = eager.step(batch, 0, masks, random_mask)
        lg = graphed.replay()
        assert le["grad_norm"] == lg["grad_norm"] and le["grad_norm"] > 0.99, (step, le["grad_norm"], lg["grad_norm"])
        seen.append(le["grad_norm"])
        for k in le:
            assert abs(le[k] - lg[k]) <= 1e-6 * max(1.0, abs(le[k])), (step, k, le[k], lg[k])
        pe, pg = model_e._flat_params(), model_g._flat_params()
        for k in keys:
            assert float((pe[k] - pg[k]).abs().max()) <= 1e-7 * max(1.0, float(pe[k].abs().max())), (step, k)
    print(f"captured clipping step: grad_norm {seen}")
    assert seen[0] != seen[1] and not graphed._recapture_pending
    graphed.max_grad_norm = 0.5
    assert graphed._recapture_pending


# ---- the stand-alone function ---------------------------------------------------------------------------------------------------------
def test_clip_grad_norm_on_the_class_api_loop(step_inputs):
    """loss.backward(); training.clip_grad_norm_(model.parameters(), 0.99) on the autograd bridge's gradients: norm and coefficient within
    1 fp32 ulp of float64, every gradient bit-equal to fp32(g * coef), parameters without a gradient ignored, no host synchronisation
    needed for the result (a device scalar)."""
    import torch.nn.functional as F
    _g, batch, masks, random_mask = step_inputs
    model, vq = common.product_models(precision="f16x3", device=DEV)
    cfg = model.config
    with torch.no_grad():
        index, latent, masked_motion = training.targets(vq, batch["motion"], batch["expressions"], batch["trans"], batch["foot_contact"])
    model.train()
    model.dropout_masks_override = [list(fm) for fm in masks]
    spk = torch.zeros(masked_motion.shape[0], 1, dtype=torch.long, device=DEV)
    seed_mask = torch.ones_like(masked_motion)
    seed_mask[:, :cfg.seed_frames] = 0
    total = 0.0
    for mask, use_audio in ((seed_mask, True), (random_mask, True), (random_mask, False)):
        out = model(batch["audio"], spk, masked_motion, mask, use_audio=use_audio)
        rec = sum(getattr(cfg, "l" + q[0]) * F.mse_loss(out[f"rec_{q}"], latent[q]) for q in ("upper", "lower", "hands", "face"))
        cls = sum(getattr(cfg, "c" + q[0]) * F.nll_loss(F.log_softmax(out[f"cls_{q}"], dim=2).reshape(-1, 256), index[q].reshape(-1))
                  for q in ("upper", "lower", "hands", "face"))
        total = total + rec + cls
    total.backward()
    model.eval()
    params = list(model.parameters())
    before = {i: p.grad.clone() for i, p in enumerate(params) if p.grad is not None}
    assert 440 < len(before) < len(params)                       # the unused template layers have no gradient
    norm = training.clip_grad_norm_(model.parameters(), 0.99)
    assert norm.is_cuda and norm.dtype == torch.float32 and norm.dim() == 0
    coef_t = training._clip_table([params[i].grad for i in before]).norm_buffers().coef.clone()
    want_n, want_c = gc.formula(sumsq64(before), 1.0, 0.99)
    copies = [torch.nn.Parameter(g.clone()) for g in before.values()]
    for p, g in zip(copies, before.values()):
        p.grad = g.clone()
    torch_norm = float(torch.nn.utils.clip_grad_norm_(copies, 0.99))
    print(f"clip_grad_norm_: norm {float(norm)!r} (float64 {want_n!r}; torch's fp32 on copies {torch_norm!r}), coef {float(coef_t)!r} (float64 {want_c!r})")
    assert abs(float(norm) - want_n) <= gc.ulp32(want_n) and abs(float(coef_t) - want_c) <= gc.ulp32(want_c)
    for i, g in before.items():
        assert torch.equal(params[i].grad, g * coef_t), i
    assert all(p.grad is None for i, p in enumerate(params) if i not in before)
    assert len(training._CLIP_TABLES) >= 1 and training._clip_table([params[i].grad for i in before]) is training._clip_table([params[i].grad for i in before])
