"""Comparison helpers shared by the float64 kernel tests (test_backward_kernels_gpu.py, test_forward_kernels_*.py, test_attention_lstm_*.py, test_gemm_float64_*.py)."""
import math

import torch

DEV = "cuda"
EPS32 = 2.0 ** -24          # unit roundoff of fp32
FAR = 8.0                   # a wrong reference must miss by more than FAR x the tolerance
SPLIT_REL = 3 * 2.0 ** -22          # per product of two split-f16 operands (EMAGE_F16X3 / EMAGE_H2)
SPLIT_FLOOR = 2.0 ** -25            # of an operand times its scale: the fp16-subnormal floor of the low plane


def _scale(ref):
    return float(ref.abs().max()) if ref.numel() else 0.0


def _cmp(name, got, ref, tol):
    """Every entry of `got` within `tol` (absolute; a number, or a tensor broadcast against the entries) of the float64 reference;
    NaN fails.  Returns the max error."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = (got - ref).abs()
    bad = int((~(err <= tol)).sum())
    mx = float(torch.nan_to_num(err, nan=math.inf).max()) if err.numel() else 0.0
    sc, tmax = _scale(ref), float(torch.as_tensor(tol).max())
    print(f"{name}: max err {mx:.3e} = {mx / sc if sc else 0.0:.2e} x scale {sc:.3e} (tol {tmax / sc if sc else 0.0:.1e} x scale)")
    assert bad == 0, f"{name}: {bad}/{err.numel()} entries outside the tolerance (at most {tmax:.3e}), max err {mx:.3e}, scale {sc:.3e}"
    return mx


def _far(name, got, wrong, tol):
    """The kernel's output is NOT the wrong reference: it misses it by more than FAR x tol (its largest value) somewhere."""
    miss = float((got.detach().double().cpu() - wrong.detach().double().cpu()).abs().max())
    tol = float(torch.as_tensor(tol).max())
    assert miss > FAR * tol, f"{name}: the wrong reference is within {miss:.3e} (tol {tol:.3e}): the data cannot tell them apart"


def _nan_outside(name, buf, *block):
    """buf (the whole NaN-filled buffer) is still NaN everywhere outside buf[block]."""
    b = buf.detach().cpu()
    keep = torch.ones(b.shape, dtype=torch.bool)
    keep[block] = False
    assert bool(torch.isnan(b[keep]).all()), f"{name}: {int((~torch.isnan(b[keep])).sum())} entries written outside the output block"


def _nans(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
