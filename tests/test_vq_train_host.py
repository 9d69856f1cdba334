"""Tokenizer training without a device: (i) the numbers tests/golden/make_golden_vq_train.py recorded from the REAL reference are
reproduced by a float64 restatement written here, with the quantiser's backward as the EXPLICIT formulas the kernels implement
(not autograd) — pins those formulas independently of the device; (ii) the host logic of pantomatrix_amd/training_vq.py (tape,
autograd bridge, the opt-in `unfreeze()` / `freeze()` state) on the CPU stand-ins of tests/fake_ops.py, with the two new ops restated
here; (iii) the new ops exist for the ROCm dispatch key only."""
import contextlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fake_ops
import vq_train_common as vc
from pantomatrix_amd import ops, training_vq


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "vq_train_step.npz"))


# ---- float64 restatement ------------------------------------------------------------------------------------------------------------
class _Quantize64(torch.autograd.Function):
    """Quantizer.forward (P:144-156) with the backward written out: dz = g_zq + g_loss beta s (z - e[idx]), dE[k] = g_loss s sum_{idx[n] = k}
    (e[k] - z[n]), s = 2 / (N D); g_zq does not reach the codebook."""

    @staticmethod
    def forward(ctx, z, e, idx, beta):
        zq = e[idx]
        ctx.save_for_backward(z, e, idx)
        ctx.beta = beta
        mse = ((zq - z) ** 2).mean()
        p = torch.bincount(idx, minlength=e.shape[0]).double() / idx.numel()
        return zq.clone(), mse + beta * mse, torch.exp(-(p * torch.log(p + 1e-10)).sum())

    @staticmethod
    def backward(ctx, g_zq, g_loss, _g_perplexity):
        z, e, idx = ctx.saved_tensors
        s = 2.0 / z.numel()
        dz = g_zq + g_loss * ctx.beta * s * (z - e[idx])
        de = torch.zeros_like(e).index_add_(0, idx, g_loss * s * (e[idx] - z))
        return dz, de, None, None


def _conv(sd, name, h):
    return F.conv1d(h, sd[name + ".weight"], sd[name + ".bias"], padding=1)


def _res(sd, name, h):
    return _conv(sd, name + ".model.2", F.leaky_relu(_conv(sd, name + ".model.0", h), 0.2)) + h


def _encoder64(sd, x, n_layer):
    h = x.transpose(1, 2)
    for i in range(n_layer):
        h = _res(sd, f"encoder.main.{3 * i + 2}", F.leaky_relu(_conv(sd, f"encoder.main.{3 * i}", h), 0.2))
    return h.transpose(1, 2)


def _decoder64(sd, z, n_layer):
    h = z.transpose(1, 2)
    for i in range(2):
        h = _res(sd, f"decoder.main.{i}", h)
    for i in range(n_layer):
        h = F.leaky_relu(_conv(sd, f"decoder.main.{2 + 2 * i}", h), 0.2)
    return _conv(sd, f"decoder.main.{2 + 2 * n_layer}", h).transpose(1, 2)


def _step64(tag, idx=None):
    """One step of the fixture's objective in float64 -> (outputs, loss, {name: gradient})."""
    cfg = vc.case_config(tag)
    sd = {k: v.double().requires_grad_(True) for k, v in vc.case_state(tag).items()}
    x = vc.case_input(tag).double()
    pre = _encoder64(sd, x, cfg["vae_layer"])
    out = {}
    if idx is not None:
        zq, emb, perp = _Quantize64.apply(pre.reshape(-1, pre.shape[-1]), sd["quantizer.embedding.weight"], idx, float(cfg["vae_quantizer_lambda"]))
        out.update(poses_feat=zq.view(pre.shape), embedding_loss=emb, perplexity=perp)
        pre = zq.view(pre.shape)
    out["rec_pose"] = _decoder64(sd, pre, cfg["vae_layer"])
    loss = F.mse_loss(out["rec_pose"], x) + (out["embedding_loss"] if idx is not None else 0.0)
    loss.backward()
    return out, loss, {k: v.grad for k, v in sd.items() if v.grad is not None}


@pytest.mark.parametrize("tag", list(vc.CASES))
def test_golden_is_reproduced_by_the_float64_restatement(golden, tag):
    g = golden
    quantized = vc.CASES[tag][0] == "vq"
    assert abs(float(vc.case_input(tag).double().sum()) - float(g[f"{tag}_x_sum"])) < 1e-9          # the seeded input is the fixture's
    idx = torch.from_numpy(g[f"{tag}_idx"].astype(np.int64)) if quantized else None
    out, loss, grads = _step64(tag, idx)
    rows = lambda t: t.detach().reshape(-1, t.shape[-1])[::int(g["row_step"])].numpy()
    # the reference ran in fp32: its distance from float64 is a few 1e-6 of each quantity's scale
    assert abs(float(loss.detach()) - float(g[f"{tag}_loss"])) < 1e-5 * abs(float(loss.detach()))
    np.testing.assert_allclose(rows(out["rec_pose"]), g[f"{tag}_rec_pose_rows"], atol=2e-5, rtol=0)
    if quantized:
        counts = torch.bincount(idx, minlength=256)
        assert int((counts == 0).sum()) >= 1 and int(counts.max()) > 8                      # the data condition the script checked
        assert abs(float(out["embedding_loss"]) - float(g[f"{tag}_embedding_loss"])) < 1e-5 * float(out["embedding_loss"])
        assert abs(float(out["perplexity"]) - float(g[f"{tag}_perplexity"])) < 1e-5 * float(out["perplexity"])
        np.testing.assert_allclose(rows(out["poses_feat"]), g[f"{tag}_poses_feat_rows"], atol=1e-5, rtol=0)
        de, ref = grads["quantizer.embedding.weight"], torch.from_numpy(g[f"{tag}_grad_codebook"]).double()
        err = float((de - ref).abs().max())
        print(f"{tag}: codebook gradient float64 formulas vs the reference's autograd: max err {err:.3e}, scale {float(ref.abs().max()):.3e}")
        assert err <= 1e-5 * float(ref.abs().max())
        assert bool((de[counts == 0] == 0).all()) and bool((ref[counts == 0] == 0).all())
    names = [str(n) for n in g[f"{tag}_grad_names"]]
    assert set(names) == set(grads)
    gmax = float(np.max(g[f"{tag}_grad_norms"]))
    for n, norm, first in zip(names, g[f"{tag}_grad_norms"], g[f"{tag}_grad_first"]):
        assert abs(float(grads[n].norm()) - float(norm)) <= 1e-4 * float(norm) + 1e-7 * gmax, n
        assert abs(float(grads[n].reshape(-1)[0]) - float(first)) <= 1e-4 * float(grads[n].abs().max()) + 1e-7 * gmax, n


# ---- host logic on the CPU stand-ins ----------------------------------------------------------------------------------------------
def _fake_quantize_train(z2d, codebook, idx, beta, zq=None, image_dtype=None, n_store=None):
    fake_ops.CALLS.append("vq_quantize_train")
    n, d = z2d.shape
    rows = codebook[idx]
    zq = rows.clone() if zq is None else zq.copy_(rows)
    image = None
    if image_dtype is not None:
        assert image_dtype == ops.F32
        image = torch.zeros(n, d if n_store is None else n_store)
        image[:, :d] = rows
    hist = torch.bincount(idx, minlength=codebook.shape[0]).to(torch.int32)
    mse = ((rows - z2d).double() ** 2).mean()
    p = hist.double() / n
    scalars = torch.stack([mse + beta * mse, torch.exp(-(p * torch.log(p + 1e-10)).sum())]).float()
    return zq, image, hist, scalars


def _fake_quantize_backward(z2d, codebook, idx, g_zq, g_loss, beta, dz=None, d_codebook=None):
    fake_ops.CALLS.append("vq_quantize_backward")
    s = 2.0 / z2d.numel()
    gl = float(g_loss)
    c = (gl * beta * s) * (z2d - codebook[idx])
    dz = c if g_zq is None else g_zq + c
    de = torch.zeros_like(codebook, dtype=torch.float64).index_add_(0, idx, (codebook[idx] - z2d).double()) * (gl * s)
    return dz, de.float()


@contextlib.contextmanager
def _installed():
    saved = ops.vq_quantize_train, ops.vq_quantize_backward
    with fake_ops.installed():
        ops.vq_quantize_train, ops.vq_quantize_backward = _fake_quantize_train, _fake_quantize_backward
        try:
            yield
        finally:
            ops.vq_quantize_train, ops.vq_quantize_backward = saved


def _class_api_step(m, x):
    """The reference's idiom on the product class -> (outputs, loss, {name: grad})."""
    opt = torch.optim.Adam(m.parameters(), lr=vc.LR, betas=vc.BETAS, eps=vc.EPS)
    opt.zero_grad()
    out = m(x)
    loss = F.mse_loss(out["rec_pose"], x) + (out["embedding_loss"] if "embedding_loss" in out else 0.0)
    loss.backward()
    grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    opt.step()
    return out, loss, grads


@pytest.mark.parametrize("tag,precision", [("vq2", "fp32"), ("vq3", "f16x3"), ("vae", "fp32"), ("vae", "f16x3")])
def test_class_api_host_logic_against_the_golden(golden, tag, precision):
    """`m.unfreeze().train(); out = m(x); loss.backward(); Adam.step()` through the tape and the autograd bridge, kernels restated on the
    CPU: outputs, loss, gradient norms, codebook gradient and post-Adam sums against the real reference's step (the bars of
    tests/test_train_forward_gpu.py for the EMAGE step)."""
    g = golden
    m = vc.product_model(tag, precision)
    x = vc.case_input(tag)
    quantized = vc.CASES[tag][0] == "vq"
    with _installed():
        if quantized:
            with torch.no_grad():
                assert np.array_equal(m.map2index(x).reshape(-1).numpy(), g[f"{tag}_idx"].astype(np.int64))
        m.unfreeze().train()
        out, loss, grads = _class_api_step(m, x)
        assert ("vq_quantize_train" in fake_ops.CALLS) == quantized and ("vq_quantize_backward" in fake_ops.CALLS) == quantized
    assert set(out) == ({"poses_feat", "embedding_loss", "perplexity", "rec_pose"} if quantized else {"rec_pose"})
    assert out["rec_pose"].requires_grad and (not quantized or (out["embedding_loss"].requires_grad and out["poses_feat"].requires_grad
                                                               and not out["perplexity"].requires_grad))
    want = float(g[f"{tag}_loss"])
    assert abs(float(loss.detach()) - want) < 2e-4 * max(1.0, abs(want))
    names = [str(n) for n in g[f"{tag}_grad_names"]]
    assert set(names) == set(grads)
    gmax = float(np.max(g[f"{tag}_grad_norms"]))
    params = dict(m.named_parameters())
    for n, norm, first, s in zip(names, g[f"{tag}_grad_norms"], g[f"{tag}_grad_first"], g[f"{tag}_param_sum_after"]):
        gn = float(grads[n].norm())
        assert abs(gn - float(norm)) <= 5e-3 * float(norm) + 1e-6 * gmax, (n, gn, float(norm))
        assert abs(float(grads[n].reshape(-1)[0]) - float(first)) <= 5e-3 * float(grads[n].abs().max()) + 1e-6 * gmax, n
        p = params[n]
        assert abs(float(p.detach().double().sum()) - float(s)) <= 3e-5 * p.numel() ** 0.5 + 2e-3, n
    if quantized:
        ref = torch.from_numpy(g[f"{tag}_grad_codebook"])
        de = grads["quantizer.embedding.weight"]
        assert float((de - ref).abs().max()) <= 1e-3 * float(ref.abs().max()) + 2e-6 * gmax
        assert bool((de[ref.abs().sum(1) == 0] == 0).all())


def test_unfreeze_and_freeze_state_logic():
    """Opt-in: a fresh tokenizer's `.train()` raises (the EMAGE trainer relies on frozen tokenizers); `unfreeze()` lifts that for the
    instance, `freeze()` restores it; eval-mode results before `unfreeze()` and after `freeze()` are the same bits."""
    for tag in ("vq2", "vae"):
        m = vc.product_model(tag, "fp32")
        xin = vc.case_input(tag)[:2, :16]
        with _installed(), torch.no_grad():
            before = m(xin)
        with pytest.raises(NotImplementedError):
            m.train()
        assert not m.training
        assert m.unfreeze() is m and not m.training            # unfreeze alone does not switch the mode
        with _installed(), torch.no_grad():
            still = m(xin)
        assert all(torch.equal(before[k], still[k]) for k in before)
        m.train()
        assert m.training
        with _installed():
            out = m(xin)
        assert out["rec_pose"].grad_fn is not None
        m.eval()
        m.train()                                              # still allowed: the instance stays trainable until freeze()
        assert m.freeze() is m and not m.training
        with pytest.raises(NotImplementedError):
            m.train()
        with _installed(), torch.no_grad():
            after = m(xin)
        assert set(after) == set(before) and all(torch.equal(before[k], after[k]) for k in before)
        other = vc.product_model(tag, "fp32")                  # the switch is per instance
        with pytest.raises(NotImplementedError):
            other.train()


def test_bf16_is_refused_like_the_emage_training_forward():
    m = vc.product_model("vq2", "bf16")
    with pytest.raises(ValueError, match="fp32-storage"):
        training_vq.TokenizerForward(m)


def test_new_ops_are_registered_for_the_rocm_key_only():
    for name in ("vq_quantize_train", "vq_quantize_backward"):
        assert hasattr(torch.ops.emage, name)
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"emage::{name}", "CUDA")
        for key in ("CPU", "CompositeImplicitAutograd", "CompositeExplicitAutograd"):
            assert not torch._C._dispatch_has_kernel_for_dispatch_key(f"emage::{name}", key), (name, key)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.vq_quantize_train(torch.zeros(4, 8), torch.zeros(2, 8), torch.zeros(4, dtype=torch.int64), 1.0)
