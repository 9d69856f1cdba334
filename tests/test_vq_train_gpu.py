"""Tokenizer training on the MI355X (csrc/vq_train.hip, pantomatrix_amd/training_vq.py).

Kernel level, self-contained: `emage_vq_quantize_train` / `emage_vq_quantize_backward` against a float64 torch-autograd restatement
of Quantizer.forward (P:144-156), with the conventions of tests/test_backward_kernels_gpu.py — outputs into NaN-filled buffers,
tolerances as a fraction of the reference's scale estimated from the arithmetic, `~(err <= tol)`, each comparison printing its max
error, and a plausible WRONG reference that must be told apart.  Model level: the class API and `TokenizerTrainer` against the
REAL reference's step (tests/golden/vq_train_step.npz) at the bars the EMAGE step uses against train_step_b2.npz."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vq_train_common as vc
from oracle import emage_oracle as orc
from pantomatrix_amd import ops, training_vq
from pantomatrix_amd._lib import BF16, F32, H2

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS32 = 2.0 ** -24
FAR = 8.0
K, D = 256, 256


def _cmp(name, got, ref, tol):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = (got - ref).abs()
    bad = int((~(err <= tol)).sum())
    mx = float(torch.nan_to_num(err, nan=math.inf).max()) if err.numel() else 0.0
    sc = float(ref.abs().max()) if ref.numel() else 0.0
    print(f"{name}: max err {mx:.3e} = {mx / sc if sc else 0.0:.2e} x scale {sc:.3e} (tol {tol / sc if sc else 0.0:.1e} x scale)")
    assert bad == 0, f"{name}: {bad}/{err.numel()} entries outside the tolerance {tol:.3e}, max err {mx:.3e}, scale {sc:.3e}"
    return mx


def _far(name, got, wrong, tol):
    miss = float((got.detach().double().cpu() - wrong.detach().double().cpu()).abs().max())
    assert miss > FAR * tol, f"{name}: the wrong reference is within {miss:.3e} (tol {tol:.3e}): the data cannot tell them apart"


def _nan_outside(name, buf, *block):
    b = buf.detach().cpu()
    keep = torch.ones(b.shape, dtype=torch.bool)
    keep[block] = False
    assert bool(torch.isnan(b[keep]).all()), f"{name}: {int((~torch.isnan(b[keep])).sum())} entries written outside the output block"


def _nans(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _reference(z, cb, idx, beta, g_zq, g_loss):
    """P:144-156 in float64 with torch autograd, the codes taken as given -> z_q, loss, perplexity, dz, dE (+ the wrong variants)."""
    zz, e = z.double().requires_grad_(), cb.double().requires_grad_()
    zq = e[idx]
    loss = torch.mean((zq - zz.detach()) ** 2) + beta * torch.mean((zq.detach() - zz) ** 2)
    st = zz + (zq - zz).detach()
    e_mean = F.one_hot(idx, cb.shape[0]).double().mean(0)
    perplexity = torch.exp(-torch.sum(e_mean * torch.log(e_mean + 1e-10)))
    total = g_loss * loss + ((st * g_zq.double()).sum() if g_zq is not None else 0.0)
    total.backward()
    dz_no_beta = g_zq.double() if g_zq is not None else torch.zeros_like(zz)                               # wrong: the commitment term forgotten
    de_leaked = e.grad + (torch.zeros_like(e).index_add_(0, idx, g_zq.double()) if g_zq is not None else 0.0)   # wrong: g_zq reaches the codebook
    return zq.detach(), loss.detach(), perplexity, zz.grad, e.grad, dz_no_beta, de_leaked


# (rows, z as a strided view, g_zq given, beta, g_loss)
KERNEL_CASES = [(64, False, True, 1.0, 0.75), (3584, True, True, 0.25, 37.5), (7680, False, True, 1.0, 3.0), (3584, False, False, 1.0, 0.75),
                (64, True, False, 0.25, 37.5)]


@pytest.mark.parametrize("n,strided,with_g,beta,g_loss", KERNEL_CASES,
                         ids=[f"n{n}{'_strided' if s else ''}{'_gzq' if w else '_nogzq'}" for n, s, w, _b, _g in KERNEL_CASES])
def test_quantize_kernels_against_float64_autograd(n, strided, with_g, beta, g_loss):
    g = torch.Generator().manual_seed(1000 + n + 7 * strided + 3 * with_g)
    # z near the codebook's scale, so that the nearest code is not a matter of |e|^2 alone; at N = 64 most codes stay unused
    z, cb = torch.randn(n, D, generator=g), torch.randn(K, D, generator=g)
    z[: n // 2] += cb[torch.randint(0, K // 4, (n // 2,), generator=g)]               # half the rows crowd a quarter of the codes
    g_zq = 1e-3 * torch.randn(n, D, generator=g) if with_g else None                 # small, so that the commitment term of dz is visible beside it
    zbuf = _nans(n + 2, D + 64)
    zbuf[:n, :D] = z.to(DEV)
    zd = zbuf[:n, :D] if strided else z.to(DEV)
    cbd = cb.to(DEV)
    idx = ops.vq_argmin(zd, cbd)
    # the codes themselves: the fp32 arg-min of P:147-149 on the CPU, every row
    assert torch.equal(idx.cpu(), orc.vq_nearest(z.unsqueeze(0), cb).reshape(-1))
    counts = torch.bincount(idx.cpu(), minlength=K)
    assert int(counts.max()) > (8 if n > 64 else 1) and (n > 64 or int((counts == 0).sum()) > 0)      # codes repeat; at N = 64 most stay unused
    zq_ref, loss_ref, perp_ref, dz_ref, de_ref, dz_wrong, de_wrong = _reference(z, cb, idx.cpu(), beta, g_zq, g_loss)

    # ---- forward: rows, operand images, histogram, the two scalars ----
    zq_buf = _nans(n + 3, D + 8)
    zq, img, hist, scalars = ops.vq_quantize_train(zd, cbd, idx, beta, zq=zq_buf[:n, :D], image_dtype=F32, n_store=D + 64)
    torch.cuda.synchronize()
    _nan_outside("zq", zq_buf, slice(0, n), slice(0, D))
    assert torch.equal(zq.cpu(), cb[idx.cpu()]) and torch.equal(img[:, :D].cpu(), cb[idx.cpu()]) and float(img[:, D:].abs().max()) == 0.0
    _, img_bf, hist2, _ = ops.vq_quantize_train(zd, cbd, idx, beta, image_dtype=BF16, n_store=D)
    assert torch.equal(img_bf.cpu(), cb[idx.cpu()].to(torch.bfloat16))
    _, img_h2, _, _ = ops.vq_quantize_train(zd, cbd, idx, beta, image_dtype=H2, n_store=D)
    _cmp("zq image (EMAGE_H2)", ops.h2_unpack(img_h2), cb[idx.cpu()], 2.0 ** -20 * float(cb.abs().max()))       # hi + lo fp16 planes: 2^-22 relative
    assert hist.dtype == torch.int32 and torch.equal(hist.cpu().long(), counts) and torch.equal(hist2, hist)
    # (e - z) is one fp32 rounding, its square and the sums are float64, the results are rounded to fp32 once: a few 2^-24 of the value
    _cmp("embedding_loss", scalars[0], loss_ref, 8 * EPS32 * float(loss_ref))
    _cmp("perplexity", scalars[1], perp_ref, 8 * EPS32 * float(perp_ref))
    _far("embedding_loss without beta", scalars[0], loss_ref / (1.0 + beta), 8 * EPS32 * float(loss_ref))

    # ---- backward: dz, dE ----
    gl = torch.tensor([g_loss], dtype=torch.float32, device=DEV)
    gbuf = _nans(n, D + 32)
    if with_g:
        gbuf[:, :D] = g_zq.to(DEV)
    dz_buf, de = _nans(n + 1, D + 16), _nans(K, D)
    ops.vq_quantize_backward(zd, cbd, idx, gbuf[:, :D] if with_g else None, gl, beta, dz=dz_buf[:n, :D], d_codebook=de)
    torch.cuda.synchronize()
    _nan_outside("dz", dz_buf, slice(0, n), slice(0, D))
    # dz: the coefficient, (z - e), their product and the add are one fp32 rounding each
    tol_dz = 8 * EPS32 * float(dz_ref.abs().max())
    _cmp("dz", dz_buf[:n, :D], dz_ref, tol_dz)
    _far("dz without the beta term", dz_buf[:n, :D], dz_wrong, tol_dz)
    # dE: every term (e - z) is one fp32 rounding (2^-24 of a term of magnitude <= max|e - z|), the sum of at most max-count terms and the
    # scaling are float64, the result is rounded to fp32 once
    tol_de = 8 * EPS32 * float(de_ref.abs().max())
    _cmp("dE", de, de_ref, tol_de)
    assert bool((de.cpu()[counts == 0] == 0).all())                                  # unused codes: exactly zero
    if with_g:
        _far("dE with g_zq leaked into it", de, de_wrong, tol_de)
    _far("dE without g_loss", de, de_ref / g_loss, tol_de)


def test_codebook_gradient_is_bit_reproducible():
    g = torch.Generator().manual_seed(5)
    n = 3584
    z, cb = torch.randn(n, D, generator=g).to(DEV), torch.randn(K, D, generator=g).to(DEV)
    g_zq, gl = torch.randn(n, D, generator=g).to(DEV), torch.tensor([1.7], device=DEV)
    idx = ops.vq_argmin(z, cb)
    runs = []
    for _ in range(2):
        _zq, _img, hist, scalars = ops.vq_quantize_train(z, cb, idx, 0.25)
        dz, de = ops.vq_quantize_backward(z, cb, idx, g_zq, gl, 0.25)
        runs.append((hist.clone(), scalars.clone(), dz.clone(), de.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_invalid_arguments_are_refused():
    from pantomatrix_amd import _lib
    lib = _lib.load()
    assert lib.emage_vq_quantize_train(None, 0, None, None, None, 0, None, 0, 0, 0, None, None, 1.0, None, 0, 0, 0, 0, None) == -1
    assert lib.emage_vq_quantize_backward(None, 0, None, None, None, 0, None, 1.0, None, 0, None, 0, 0, 0, None) == -1
    z, cb = torch.zeros(32, D, device=DEV), torch.zeros(K, D, device=DEV)
    idx = torch.zeros(32, dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.EmageKernelError):       # a workspace that is too small
        ops._vq_quantize_train(z, cb, idx, torch.empty(32, D, device=DEV), None, F32, torch.empty(K, dtype=torch.int32, device=DEV),
                               torch.empty(2, device=DEV), 1.0, torch.empty(1, dtype=torch.float64, device=DEV))


# ---- model level ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "vq_train_step.npz"))


def _class_api_step(m, x):
    opt = torch.optim.Adam(m.parameters(), lr=vc.LR, betas=vc.BETAS, eps=vc.EPS)
    opt.zero_grad()
    out = m(x)
    loss = F.mse_loss(out["rec_pose"], x) + (out["embedding_loss"] if "embedding_loss" in out else 0.0)
    loss.backward()
    grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    opt.step()
    return out, loss, grads


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("tag", list(vc.CASES))
def test_class_api_step_matches_the_reference(golden, tag, precision):
    """`m.unfreeze().train(); out = m(x); loss.backward(); torch.optim.Adam.step()` on the device against the REAL reference's step:
    codes, outputs, loss, every gradient's norm and first element, the whole codebook gradient, post-Adam parameter sums."""
    g = golden
    quantized = vc.CASES[tag][0] == "vq"
    m = vc.product_model(tag, precision, DEV)
    x = vc.case_input(tag).to(DEV)
    if quantized:
        with torch.no_grad():
            assert torch.equal(m.map2index(x).reshape(-1).cpu(), torch.from_numpy(g[f"{tag}_idx"].astype(np.int64)))
    before = {k: v.clone() for k, v in m._flat_params().items()}
    m.unfreeze().train()
    out, loss, grads = _class_api_step(m, x)
    step = int(g["row_step"])
    rows = lambda t: t.detach().reshape(-1, t.shape[-1])[::step].cpu().numpy()
    assert set(out) == ({"poses_feat", "embedding_loss", "perplexity", "rec_pose"} if quantized else {"rec_pose"})
    err = float(np.abs(rows(out["rec_pose"]) - g[f"{tag}_rec_pose_rows"]).max())
    print(f"{tag} {precision}: rec_pose max err {err:.3e}")
    assert err <= 3e-4                                                                   # the eval-mode parity bar of the same stacks
    want = float(g[f"{tag}_loss"])
    print(f"{tag} {precision}: loss {float(loss.detach()):.7f} vs {want:.7f}")
    assert abs(float(loss.detach()) - want) < 2e-4 * max(1.0, abs(want))
    if quantized:
        assert not out["perplexity"].requires_grad and out["embedding_loss"].requires_grad and out["poses_feat"].requires_grad
        np.testing.assert_allclose(rows(out["poses_feat"]), g[f"{tag}_poses_feat_rows"], atol=1e-5, rtol=0)
        for k in ("embedding_loss", "perplexity"):
            assert abs(float(out[k]) - float(g[f"{tag}_{k}"])) < 2e-4 * max(1.0, abs(float(g[f"{tag}_{k}"]))), k
    names = [str(n) for n in g[f"{tag}_grad_names"]]
    assert set(names) == set(grads)
    gmax = float(np.max(g[f"{tag}_grad_norms"]))
    params = m._flat_params()
    worst = 0.0
    for n, norm, first, s in zip(names, g[f"{tag}_grad_norms"], g[f"{tag}_grad_first"], g[f"{tag}_param_sum_after"]):
        gn = float(grads[n].norm())
        worst = max(worst, abs(gn - float(norm)) / (float(norm) + 1e-3 * gmax))
        assert abs(gn - float(norm)) <= 5e-3 * float(norm) + 1e-6 * gmax, (n, gn, float(norm))
        assert abs(float(grads[n].reshape(-1)[0]) - float(first)) <= 5e-3 * float(grads[n].abs().max()) + 1e-6 * gmax, n
        p = params[n]
        assert abs(float(p.double().sum()) - float(s)) <= 3e-5 * p.numel() ** 0.5 + 2e-3, n
        assert not torch.equal(p, before[n]), n
    print(f"{tag} {precision}: {len(names)} gradient norms, worst relative error {worst:.2e}")
    if quantized:
        ref = torch.from_numpy(g[f"{tag}_grad_codebook"])
        de = grads["quantizer.embedding.weight"].cpu()
        err = float((de - ref).abs().max())
        print(f"{tag} {precision}: codebook gradient max err {err:.3e}, scale {float(ref.abs().max()):.3e}")
        assert err <= 1e-3 * float(ref.abs().max()) + 2e-6 * gmax                        # compare_grads(rel=1e-3)
        assert bool((de[ref.abs().sum(1) == 0] == 0).all())


@pytest.mark.parametrize("tag,precision", [("vq2", "f16x3"), ("vq3", "fp32"), ("vae", "f16x3")])
def test_trainer_step_equals_the_class_api_step_and_is_bit_reproducible(tag, precision):
    """`TokenizerTrainer.step` (no torch autograd, `emage_adam_multi`) lands where the class API + torch.optim.Adam lands; two runs from
    the same state give the same bits; the eval-mode forward afterwards runs on the updated weights (the re-pack happened)."""
    x = vc.case_input(tag).to(DEV)
    quantized = vc.CASES[tag][0] == "vq"
    ref_model = vc.product_model(tag, precision, DEV)
    ref_model.unfreeze().train()
    _out, loss, _grads = _class_api_step(ref_model, x)
    runs = []
    for _ in range(2):
        m = vc.product_model(tag, precision, DEV)
        with torch.no_grad():
            code0 = m.map2index(x).clone() if quantized else m(x)["rec_pose"].clone()     # packs the eval operands from the initial weights
        trainer = training_vq.TokenizerTrainer(m, lr=vc.LR, betas=vc.BETAS, eps=vc.EPS)
        res = trainer.step(x)
        runs.append((m, res, code0))
    (m1, res1, code0), (m2, res2, _c) = runs
    assert res1 == res2
    print(f"{tag} {precision}: trainer losses {res1}, class API loss {float(loss.detach()):.7f}")
    assert abs(res1["all"] - float(loss.detach())) <= 1e-6 * max(1.0, abs(float(loss.detach())))
    p1, p2, pr = m1._flat_params(), m2._flat_params(), ref_model._flat_params()
    worst = 0.0
    for n in p1:
        assert torch.equal(p1[n], p2[n]), n
        worst = max(worst, float((p1[n] - pr[n]).abs().max()))
    # Adam's first step moves every entry by lr g / (|g| + eps): the two paths differ in the last bits of g (the loss gradient is one kernel
    # here, torch autograd there), which matters only where |g| ~ eps — a small fraction of lr
    print(f"{tag} {precision}: max |trainer - class API| over the parameters {worst:.3e} (lr {vc.LR})")
    assert worst <= 0.05 * vc.LR
    m1.freeze()
    fresh = vc.product_model(tag, precision, DEV)
    fresh.load_state_dict(m1.state_dict())
    with torch.no_grad():
        if quantized:
            assert torch.equal(m1.map2index(x), fresh.map2index(x))
            a, b = m1(x)["rec_pose"], fresh(x)["rec_pose"]
        else:
            a, b = m1(x)["rec_pose"], fresh(x)["rec_pose"]
            assert float((a - code0).abs().max()) > 0.0
    assert torch.equal(a, b)


def test_opt_in_on_the_device():
    """A fresh tokenizer's `.train()` still raises; after `unfreeze()` it does not; `freeze()` restores the raise; eval outputs before
    `unfreeze()` and after `freeze()` are the same bits."""
    for tag in ("vq2", "vae"):
        m = vc.product_model(tag, "f16x3", DEV)
        x = vc.case_input(tag).to(DEV)
        with torch.no_grad():
            before = {k: v.clone() for k, v in m(x).items()}
            codes = m.map2index(x).clone() if tag == "vq2" else None
        with pytest.raises(NotImplementedError):
            m.train()
        m.unfreeze().train()
        out = m(x)
        assert m.training and out["rec_pose"].grad_fn is not None
        m.freeze()
        assert not m.training
        with pytest.raises(NotImplementedError):
            m.train()
        with torch.no_grad():
            after = m(x)
            assert all(torch.equal(before[k], after[k]) for k in before)
            if codes is not None:
                assert torch.equal(m.map2index(x), codes)
