"""TEST-ONLY CPU stand-ins of the gradient-norm entry points (include/emage_hip.h: emage_grad_sumsq_multi, emage_scale_multi,
emage_adam_multi_scaled), in the manner of tests/fake_ops.py and attached to it at import time: `fake_ops.grad_norm`, `fake_ops.scale_multi`
and `fake_ops.adam_multi_scaled`.  `installed()` is `fake_ops.installed()` plus these three (with `adam_multi` taking `grad_scale_dev`);
every call is recorded in `fake_ops.CALLS` under the names in `NEW_CALLS`."""
import contextlib
import types

import numpy as np
import torch

import fake_ops
from pantomatrix_amd import ops

NEW_CALLS = ("grad_norm", "scale_multi", "adam_multi_scaled")


def _buffers(tab, out):
    if out is not None:
        return out
    if getattr(tab, "_norm_fake", None) is None:
        n = len(tab.keep)
        scalars = torch.zeros(2, dtype=torch.float32)
        tab._norm_fake = types.SimpleNamespace(tensor_sumsq=torch.zeros(n, dtype=torch.float64), total_sumsq=torch.zeros(1, dtype=torch.float64),
                                               scalars=scalars, norm=scalars[0:1], coef=scalars[1:2])
    return tab._norm_fake


def new_buffers(tab):
    """A second set of outputs for the same table (the bit-reproducibility check launches twice into different buffers)."""
    if isinstance(tab, ops.AdamTable) and tab.table.is_cuda:
        return ops.GradNorm(tab)
    saved, tab._norm_fake = getattr(tab, "_norm_fake", None), None
    try:
        return _buffers(tab, None)
    finally:
        tab._norm_fake = saved


def grad_norm(tab, pre_scale=1.0, max_norm=None, out=None):
    """emage_grad_sumsq_multi: float64 sums of exact squares per tensor and over the table (torch's float64 sum: some fixed order), then
    norm and coef from the formula of the header, in double, rounded to fp32 once."""
    fake_ops.CALLS.append("grad_norm")
    out = _buffers(tab, out)
    for i, (_p, g, _m, _v) in enumerate(tab.keep):
        out.tensor_sumsq[i] = (g.detach().double() ** 2).sum()
    out.total_sumsq[0] = out.tensor_sumsq.sum()
    with np.errstate(all="ignore"):
        nrm = np.float64(pre_scale) * np.sqrt(np.float64(out.total_sumsq[0]))
        cf = np.float64(1.0)
        mx = 0.0 if max_norm is None else float(max_norm)
        if mx > 0 and not np.isinf(mx):
            cf = np.float64(mx) / (nrm + 1e-6)
            if cf > 1.0:
                cf = np.float64(1.0)
        out.norm[0] = float(np.float32(nrm))
        out.coef[0] = float(np.float32(cf))
    return out


def scale_multi(tab, coef):
    fake_ops.CALLS.append("scale_multi")
    assert coef.dtype == torch.float32 and coef.numel() == 1
    for _p, g, _m, _v in tab.keep:
        g.mul_(coef.reshape(()))


def adam_multi(tab, step, lr=1.5e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, grad_scale=1.0, zero_grad=False, skip=None, grad_scale_dev=None):
    """`fake_ops.adam_multi`; with grad_scale_dev the factor is the fp32 product grad_scale * coef, as the kernel forms it."""
    if grad_scale_dev is None:
        return fake_ops.adam_multi(tab, step, lr, beta1, beta2, eps, weight_decay, grad_scale, zero_grad, skip)
    assert grad_scale_dev.dtype == torch.float32 and grad_scale_dev.numel() == 1
    with np.errstate(all="ignore"):
        s = float(np.float32(grad_scale) * np.float32(float(grad_scale_dev)))
    fake_ops.adam_multi(tab, step, lr, beta1, beta2, eps, weight_decay, s, zero_grad, skip)
    fake_ops.CALLS[-1] = "adam_multi_scaled"


fake_ops.grad_norm, fake_ops.scale_multi, fake_ops.adam_multi_scaled = grad_norm, scale_multi, adam_multi


@contextlib.contextmanager
def installed():
    """`fake_ops.installed()` with the gradient-norm stand-ins patched into pantomatrix_amd.ops as well."""
    names = {"grad_norm": grad_norm, "scale_multi": scale_multi, "adam_multi": adam_multi}
    with fake_ops.installed():
        saved = {n: getattr(ops, n) for n in names}
        try:
            for n, f in names.items():
                setattr(ops, n, f)
            yield
        finally:
            for n, f in saved.items():
                setattr(ops, n, f)
