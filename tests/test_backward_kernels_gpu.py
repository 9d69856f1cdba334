"""The backward kernels of the training step (csrc/train_backward.hip; the loss gradients: csrc/train.hip), each called through
pantomatrix_amd.ops on the MI355X, against float64 torch autograd on the CPU of the forward operation the kernel differentiates — at the shapes the step runs, at ragged and
degenerate shapes, and at the edges where such kernels go wrong (peaked softmax rows, large row means, chunk boundaries of the
float64 reductions, padding columns).

Conventions of every case:
  * seeded inputs; outputs written into views of larger buffers pre-filled with NaN: the entries outside the written block must
    still be NaN afterwards, and a NaN inside it fails the comparison;
  * the tolerance is a fraction of the reference output's scale (its largest magnitude), estimated from the kernel's arithmetic
    (fp32 operations, fp32 or float64 accumulation) and never looser than 1e-4 of that scale; every comparison prints its max error;
  * each test also computes a plausible WRONG reference (a bug the kernel could have) and asserts that the kernel is far outside
    the tolerance of it: the data really exercises the feature."""
import math

import pytest
import torch
import torch.nn.functional as tf

from pantomatrix_amd import _lib, ops
from pantomatrix_amd._lib import EmageKernelError

from kernel_checks import DEV, EPS32, FAR, _cmp, _far, _nan_outside, _nans, _scale  # noqa: F401

pytestmark = pytest.mark.gpu


def _g(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------------------------
# attention backward: dq, dk, dv of  out = (softmax(q k^T / sqrt(hd)) * mask) v  per (batch, head)
# ---------------------------------------------------------------------------------------------------------------------------------

def _attn_inputs(b, h, tq, tk, hd, masked, seed, q_gain=1.0):
    g = _g(seed)
    q = torch.randn(b * tq, h * hd, generator=g) * q_gain
    k = torch.randn(b * tk, h * hd, generator=g)
    v = torch.randn(b, h, tk, hd, generator=g)                                   # V[b, h, j, d]
    d_out = torch.randn(b * tq, h * hd, generator=g)
    pm = (torch.rand(b, h, tq, tk, generator=g) >= 0.1).float() / 0.9 if masked else None      # dropout p = 0.1: {0, 1/0.9}
    return q, k, v, d_out, pm


def _attn_ref(q, k, v, d_out, pm, b, h, tq, tk, hd, head0_mask=False):
    """float64 autograd -> (dq, dk, dv) in the kernel's row layouts, plus (P, dS) of the float64 run for the wrong variants."""
    rows = lambda t, n: t.double().view(b, n, h, hd).permute(0, 2, 1, 3).contiguous()
    Q, K, V = rows(q, tq).requires_grad_(), rows(k, tk).requires_grad_(), v.double().requires_grad_()
    s = Q @ K.transpose(-1, -2) / math.sqrt(hd)
    s.retain_grad()
    p = torch.softmax(s, dim=-1)
    if pm is not None:
        mk = pm.double()
        if head0_mask:
            mk = mk[:, :1].expand_as(mk)
        out = (p * mk) @ V
    else:
        out = p @ V
    out.backward(rows(d_out, tq))
    back = lambda t, n: t.permute(0, 2, 1, 3).reshape(b * n, h * hd)
    return back(Q.grad, tq), back(K.grad, tk), back(V.grad, tk), p.detach(), s.grad.detach(), Q.detach(), rows(d_out, tq)


def _vt_buffer(v, b, h, tk, hd, vt_rows, ldvt):
    """V^T as the kernel reads it: vt[b][h * hd + d][j], (B, vt_rows, ldvt) with NaN in the rows and columns beyond the data."""
    vt = _nans(b, vt_rows, ldvt)
    vt[:, :h * hd, :tk] = v.permute(0, 1, 3, 2).reshape(b, h * hd, tk).to(DEV)
    return vt


def _attn_run(q, k, d_out, vt, vt_rows, pm, b, h, tq, tk, hd, ld):
    """q, k, d_out as column blocks [q | k | dO] of ONE buffer of row pitch `ld` (the step's fused qkv layout); dq, dk, dv written into
    column blocks of wider NaN buffers with spare rows.  -> (dq, dk, dv) on the CPU, after checking the buffers' untouched parts."""
    w = h * hd
    fused = _nans(b * max(tq, tk), ld)
    fused[:b * tq, :w] = q.to(DEV)
    fused[:b * tk, w:2 * w] = k.to(DEV)
    fused[:b * tq, 2 * w:3 * w] = d_out.to(DEV)
    gq, gk, gv = _nans(b * tq + 3, 3 * w + 5), _nans(b * tk + 3, 3 * w + 5), _nans(b * tk + 3, 3 * w + 5)
    blocks = ((gq, slice(0, b * tq), slice(w, 2 * w)), (gk, slice(0, b * tk), slice(2 * w, 3 * w)), (gv, slice(0, b * tk), slice(0, w)))
    views = [buf[r, c] for buf, r, c in blocks]
    ops.attention_backward(fused[:b * tq, :w], fused[:b * tk, w:2 * w], vt, vt_rows, None if pm is None else pm.to(DEV),
                           fused[:b * tq, 2 * w:3 * w], *views, b, h, tq, tk, hd)
    torch.cuda.synchronize()
    for nm, (buf, r, c) in zip(("dq", "dk", "dv"), blocks):
        _nan_outside(nm, buf, r, c)
    return [t.cpu() for t in views]


# exact-fp32 kernels (MFMA v_mfma_f32_16x16x4f32 or fmaf chains; fp32 softmax): the scores are 192-term dot products
# (error ~ sqrt(192) * 2^-24 * |q||k|/sqrt(hd) ~ 1e-6 of a unit score), which reach P through exp (relative error = the score's absolute
# error) and dS = P (dP - rowsum) a second time through dP; dq, dk, dv are 64-term sums of those.  Estimated ~1e-5 of the output scale;
# with the scores scaled 8x (peaked rows) the score error grows 8x.
ATTN_TOL, ATTN_TOL_PEAKED = 2e-5, 6e-5


MFMA_CASES = [(1, True, False), (1, False, False), (3, True, False), (3, False, False), (1, True, True), (3, False, True)]


@pytest.mark.parametrize("b,masked,peaked", MFMA_CASES,
                         ids=[f"b{b}_{'dropout' if mk else 'nomask'}{'_peaked' if pk else ''}" for b, mk, pk in MFMA_CASES])
def test_attention_backward_mfma_path(b, masked, peaked):
    """The path every attention of a training step takes (train_backward.hip: emage_attention_backward sends Tq = Tk = 64, hd = 192 with
    16-byte aligned operands and every leading dimension % 4 == 0 to attention_backward_mfma_kernel): H = 4 heads, q / k / dO as column
    blocks of one ld = 2304 buffer, V^T with spare rows (vt_rows > H hd) and ldvt in {64, 96}.  The SAME data with a leading dimension
    that is not a multiple of 4 takes the scalar kernel: both match float64 and each other."""
    h, t, hd = 4, 64, 192
    tol_rel = ATTN_TOL_PEAKED if peaked else ATTN_TOL
    q, k, v, d_out, pm = _attn_inputs(b, h, t, t, hd, masked, seed=10 * b + masked + 2 * peaked, q_gain=8.0 if peaked else 1.0)
    dq_r, dk_r, dv_r, p, ds, Q, dO = _attn_ref(q, k, v, d_out, pm, b, h, t, t, hd)
    ldvt = 96 if b == 3 else 64
    vt = _vt_buffer(v, b, h, t, hd, h * hd + 40, ldvt)
    assert 3 * h * hd == 2304
    mfma = _attn_run(q, k, d_out, vt, h * hd + 40, pm, b, h, t, t, hd, ld=2304)             # aligned: the MFMA kernel
    scalar = _attn_run(q, k, d_out, vt, h * hd + 40, pm, b, h, t, t, hd, ld=2305)           # ld % 4 != 0: the scalar kernel
    tols = [tol_rel * _scale(r) for r in (dq_r, dk_r, dv_r)]
    for path, got in (("mfma", mfma), ("scalar", scalar)):
        for nm, gt, rf, tol in zip(("dq", "dk", "dv"), got, (dq_r, dk_r, dv_r), tols):
            _cmp(f"attention[{path}].{nm}", gt, rf, tol)
    for nm, a, s, tol in zip(("dq", "dk", "dv"), mfma, scalar, tols):
        _cmp(f"attention mfma vs scalar.{nm}", a, s.double(), tol)
    # wrong references
    back = lambda t4: t4.permute(0, 2, 1, 3).reshape(b * t, h * hd)
    dk_transposed = back(ds / math.sqrt(hd) @ Q)                      # dK = dS Q instead of dS^T Q (a transposed dS block)
    _far("attention.dk vs transposed dS", mfma[1], dk_transposed, tols[1])
    if masked:
        dv_nomask = back(p.transpose(-1, -2) @ dO)                    # the mask left out of dV
        _far("attention.dv vs dV without the mask", mfma[2], dv_nomask, tols[2])
        wrong = _attn_ref(q, k, v, d_out, pm, b, h, t, t, hd, head0_mask=True)      # head 0's mask for every head
        for nm, gt, wr, tol in zip(("dq", "dk", "dv"), mfma, wrong[:3], tols):
            _far(f"attention.{nm} vs head-0 mask", gt, wr, tol)


SCALAR_SHAPES = [(64, 65, 192), (1, 1, 192), (1, 64, 192), (64, 1, 192), (33, 97, 64), (10, 11, 7), (128, 144, 16)]


@pytest.mark.parametrize("shape", SCALAR_SHAPES, ids=[f"{a}x{b}x{c}" for a, b, c in SCALAR_SHAPES])
def test_attention_backward_scalar_shapes(shape):
    """The scalar kernel (any Tq, Tk, hd; P and dS in 2 Tq Tk floats of LDS) with the dropout mask, B = 2, H = 2; (128, 144) fills the
    144 KB limit exactly.  Wrong reference: the mask left out of dV."""
    tq, tk, hd = shape
    b, h = 2, 2
    assert 2 * tq * tk * 4 <= 144 * 1024
    q, k, v, d_out, pm = _attn_inputs(b, h, tq, tk, hd, True, seed=tq * 1000 + tk)
    dq_r, dk_r, dv_r, p, _ds, _Q, dO = _attn_ref(q, k, v, d_out, pm, b, h, tq, tk, hd)
    vt = _vt_buffer(v, b, h, tk, hd, h * hd + 3, tk + 3)
    got = _attn_run(q, k, d_out, vt, h * hd + 3, pm, b, h, tq, tk, hd, ld=3 * h * hd + 1)
    tols = [ATTN_TOL * _scale(r) for r in (dq_r, dk_r, dv_r)]
    for nm, gt, rf, tol in zip(("dq", "dk", "dv"), got, (dq_r, dk_r, dv_r), tols):
        _cmp(f"attention[{tq}x{tk}x{hd}].{nm}", gt, rf, tol)
    back = lambda t4: t4.permute(0, 2, 1, 3).reshape(b * tk, h * hd)
    _far("attention.dv vs dV without the mask", got[2], back(p.transpose(-1, -2) @ dO), tols[2])


def test_attention_backward_refuses_more_than_144_kb_of_scores():
    b, h, tq, tk, hd = 1, 1, 129, 144, 16
    assert 2 * tq * tk * 4 > 144 * 1024
    q, k, d_out = _nans(b * tq, h * hd), _nans(b * tk, h * hd), _nans(b * tq, h * hd)
    vt = _nans(b, h * hd, tk)
    out = [_nans(b * tq, h * hd), _nans(b * tk, h * hd), _nans(b * tk, h * hd)]
    with pytest.raises(EmageKernelError):
        ops.attention_backward(q, k, vt, h * hd, None, d_out, *out, b, h, tq, tk, hd)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in out)


# ---------------------------------------------------------------------------------------------------------------------------------
# LayerNorm backward: dx, dgamma, dbeta of LayerNorm(x) * gamma + beta over the rows of x
# ---------------------------------------------------------------------------------------------------------------------------------

# fp32 row sums of C values (64 lane partials + a shuffle tree) for the mean, the variance and the two dx reductions: a few 1e-7 of the
# row's scale, amplified little by dx = rstd (g - mean g - xhat mean(g xhat)); dgamma / dbeta add fp32 products in float64.
LN_TOL = 2e-5
# x = 1e3 + randn: the fp32 row sum (lane partials ~1e3 C / 64, a shuffle tree up to 1e3 C) rounds at ~ulp(1e3 C), so mu is off by
# ~0.05 / C ~ 4e-5 (C = 768-1536) — a constant shift of every xhat of its row (x - mu itself is exact); dgamma = sum dy xhat inherits it.
LN_TOL_LARGE_MEAN = 1e-4
LN_C = [1, 37, 64, 768, 1000, 1024, 1025, 1536]
LN_M = [1, 3, 77, 4101]
LN_FORMS = [16, 4, False]          # ops.FUSED_LAYERNORM_BACKWARD: the fused kernel with 16 / 4 rows per block, or the row kernel + column sums


def _ln_ref(x, gamma, dy, eps, unbiased=False):
    xd, gd = x.double().requires_grad_(), gamma.double().requires_grad_()
    bd = torch.zeros_like(gd, requires_grad=True)
    if unbiased:                                                     # the wrong variant: the unbiased variance in the normalisation
        mu = xd.mean(dim=1, keepdim=True)
        y = (xd - mu) / torch.sqrt(xd.var(dim=1, unbiased=True, keepdim=True) + eps) * gd + bd
    else:
        y = tf.layer_norm(xd, (x.shape[1],), gd, bd, eps)
    y.backward(dy.double())
    return xd.grad, gd.grad, bd.grad


def _ln_case(m, c, seed, large_mean=False):
    g = _g(seed)
    xb, dyb = torch.randn(m, c + 13, generator=g), torch.randn(m, c + 6, generator=g)
    if large_mean:
        xb += 1e3
    x, dy = xb[:, 5:5 + c], dyb[:, 3:3 + c]                          # row-strided, unaligned views
    gamma = 1.0 + 0.3 * torch.randn(c, generator=g)
    init_g, init_b = torch.randn(c, generator=g), torch.randn(c, generator=g)
    return xb, dyb, x, dy, gamma, init_g, init_b


def _ln_check(m, c, seed, tol_rel, large_mean=False):
    eps = 1e-5
    xb, dyb, x, dy, gamma, init_g, init_b = _ln_case(m, c, seed, large_mean)
    dx_r, dg_r, db_r = _ln_ref(x, gamma, dy, eps)
    # one column: xhat = 0, so dx = rstd (g - g) and dgamma = sum dy xhat are 0 up to float64 noise; their scales are then those of the
    # terms, |rstd dy gamma| and |sum dy|
    term = float(dy.abs().max() * gamma.abs().max()) / math.sqrt(eps)
    tdx = tol_rel * (_scale(dx_r) if c > 1 else term)
    tdg, tdb = tol_rel * _scale(dg_r if c > 1 else db_r), tol_rel * _scale(db_r)
    xd, dyd = xb.to(DEV)[:, 5:5 + c], dyb.to(DEV)[:, 3:3 + c]
    gd = gamma.to(DEV)
    saved = ops.FUSED_LAYERNORM_BACKWARD
    results = []
    try:
        for form in LN_FORMS:
            ops.FUSED_LAYERNORM_BACKWARD = form
            tag = f"layernorm[m{m} c{c} {'fused' + str(form) if form else 'rows'}{' mean1e3' if large_mean else ''}]"
            # public entry: fresh affine gradients, and gradients ADDED to existing accumulators (views of NaN buffers)
            dx, dg, db = ops.layernorm_backward(xd, gd, dyd, eps)
            acc_g, acc_b = _nans(c + 9), _nans(c + 9)
            acc_g[4:4 + c], acc_b[4:4 + c] = init_g.to(DEV), init_b.to(DEV)
            dx2, dg2, db2 = ops.layernorm_backward(xd, gd, dyd, eps, dgamma=acc_g[4:4 + c], dbeta=acc_b[4:4 + c])
            # the kernels themselves on a NaN-filled dx window (the public entry allocates dx)
            dxb = _nans(m + 2, c + 7)
            if form and c <= 1024:
                rows = 4 if form == 4 else 16
                ws = torch.empty(((m + rows - 1) // rows) * 2 * c, dtype=torch.float64, device=DEV)
                g3, b3 = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
                ops._layernorm_backward_affine(xd, gd, dyd, eps, dxb[1:1 + m, 3:3 + c], g3, b3, False, rows, ws)
            else:
                tb = _nans(m + 2, c + 7)
                ops._layernorm_backward(xd, gd, dyd, eps, dxb[1:1 + m, 3:3 + c], tb[1:1 + m, 3:3 + c])
                torch.cuda.synchronize()
                _nan_outside(tag + ".dy_xhat", tb, slice(1, 1 + m), slice(3, 3 + c))
            torch.cuda.synchronize()
            assert dg2.data_ptr() == acc_g[4:].data_ptr() and db2.data_ptr() == acc_b[4:].data_ptr()
            _nan_outside(tag + ".dgamma accumulator", acc_g, slice(4, 4 + c))
            _nan_outside(tag + ".dbeta accumulator", acc_b, slice(4, 4 + c))
            _nan_outside(tag + ".dx", dxb, slice(1, 1 + m), slice(3, 3 + c))
            _cmp(tag + ".dx", dx, dx_r, tdx)
            _cmp(tag + ".dx (window)", dxb[1:1 + m, 3:3 + c], dx_r, tdx)
            _cmp(tag + ".dgamma", dg, dg_r, tdg)
            _cmp(tag + ".dbeta", db, db_r, tdb)
            acc_ref_g, acc_ref_b = init_g.double() + dg_r, init_b.double() + db_r
            _cmp(tag + ".dgamma accumulated", dg2, acc_ref_g, tdg + 2 * EPS32 * _scale(acc_ref_g))
            _cmp(tag + ".dbeta accumulated", db2, acc_ref_b, tdb + 2 * EPS32 * _scale(acc_ref_b))
            assert torch.equal(dx, dx2)
            results.append(dx.cpu())
    finally:
        ops.FUSED_LAYERNORM_BACKWARD = saved
    return x, dy, gamma, tdx, results


@pytest.mark.parametrize("c", LN_C)
def test_layernorm_backward(c):
    """Every form (the fused kernel with 16 and 4 rows per block — C <= 1024, LNB_MAXJ = 16 lanes of 64 columns — and the row kernel with
    two column sums, which ops takes above 1024 columns whatever the switch says), C ragged / 1024 / 1025 / 1536, M = 1 .. 4101, row-strided
    x and dy, accumulation into existing dgamma / dbeta.  Wrong reference: the unbiased variance in the normalisation (needs C > 1)."""
    for m in LN_M:
        x, dy, gamma, tdx, outs = _ln_check(m, c, seed=c * 10 + m, tol_rel=LN_TOL)
        if c > 1 and m == 77:
            wrong = _ln_ref(x, gamma, dy, 1e-5, unbiased=True)[0]
            for dx in outs:
                _far(f"layernorm[m{m} c{c}].dx vs unbiased variance", dx, wrong, tdx)


@pytest.mark.parametrize("c", [768, 1536])
def test_layernorm_backward_large_row_mean(c):
    """x = 1e3 + randn: the mean and variance of each row in fp32 (the fused form at 768, the row kernel at 1536).  Wrong reference: the
    variance as E[x^2] - E[x]^2 in fp32 (the cancellation a two-pass row kernel avoids)."""
    eps = 1e-5
    x, dy, gamma, tdx, outs = _ln_check(77, c, seed=7 + c, tol_rel=LN_TOL_LARGE_MEAN, large_mean=True)
    x32 = x.contiguous()
    var_w = ((x32 * x32).mean(dim=1, keepdim=True) - x32.mean(dim=1, keepdim=True) ** 2).double().clamp(min=eps)
    xd, g = x.double(), dy.double() * gamma.double()
    rstd = 1.0 / torch.sqrt(var_w + eps)
    xh = (xd - xd.mean(dim=1, keepdim=True)) * rstd
    wrong = rstd * (g - g.mean(dim=1, keepdim=True) - xh * (g * xh).mean(dim=1, keepdim=True))
    for dx in outs:
        _far(f"layernorm[m77 c{c} mean1e3].dx vs one-pass fp32 variance", dx, wrong, tdx)


# ---------------------------------------------------------------------------------------------------------------------------------
# BatchNorm (training) backward: dx, dgamma, dbeta of batch_norm(x, batch statistics) * gamma + beta over the rows of x
# ---------------------------------------------------------------------------------------------------------------------------------

# dgamma / dbeta: float64 sums of fp32 products (~1e-7 relative).  dx = gamma rstd (dy - sum_dy / n - xhat sum_dyxhat / n): a few fp32
# roundings of terms of size |gamma rstd dy|.  With two rows dx cancels to O(eps / var) of those terms: its tolerance is then taken per
# channel from the terms' size instead of from dx.
BN_TOL = 1e-5
BN_M = [2, 63, 64 * 512 + 1, 400003]        # 64 x 512 + 1 and 400 003 rows: chunks of 68 / 784 rows (stat_rows), a ragged last chunk
BN_C = [1, 64, 100, 512]


def _bn_ref(x, gamma, dy, eps):
    xd, gd = x.double().requires_grad_(), gamma.double().requires_grad_()
    bd = torch.zeros_like(gd, requires_grad=True)
    y = tf.batch_norm(xd, None, None, gd, bd, training=True, eps=eps)
    y.backward(dy.double())
    return xd.grad, gd.grad, bd.grad


@pytest.mark.parametrize("m", BN_M)
def test_bn_backward(m):
    """`bn_backward` and its split form `bn_backward_sums` + `bn_backward_apply` (SyncBatchNorm: the sums are all-reduced between them
    and `count` is the GLOBAL row count): strided views, one to 400 003 rows.  Two "ranks": the rows split in two, the sums of both shards
    added on the host, each shard applied with count = the total — the concatenated dx is float64 autograd over all rows.  Wrong
    reference: count = the shard's own rows."""
    eps = 1e-5
    for c in (BN_C if m < 400003 else [1, 64]):
        g = _g(m + c)
        xb, dyb = torch.randn(m, c + 3, generator=g) * 2.0 + 1.5, torch.randn(m, c + 5, generator=g)
        if m == 2:          # on a 1/16 grid the fp32 mean and variance handed to the kernel are exact (two close rows would turn their
            xb = torch.round(xb * 16.0) / 16.0          # rounding into a large relative error of xhat, which is no error of the kernel)
        x, dy = xb[:, 1:1 + c], dyb[:, 2:2 + c]
        gamma = 1.0 + 0.5 * torch.randn(c, generator=g)
        mean = x.double().mean(dim=0)
        var = x.double().var(dim=0, unbiased=False)
        dx_r, dg_r, db_r = _bn_ref(x, gamma, dy, eps)
        term = gamma.double().abs() / torch.sqrt(var + eps) * dy.double().abs().max(dim=0).values           # per channel
        tdx = BN_TOL * (_scale(dx_r) if m > 2 else term)
        tdg, tdb = BN_TOL * _scale(dg_r), BN_TOL * _scale(db_r)
        xd, dyd = xb.to(DEV)[:, 1:1 + c], dyb.to(DEV)[:, 2:2 + c]
        mean_d, var_d, gd = mean.float().to(DEV), var.float().to(DEV), gamma.to(DEV)
        ws = lambda rows: torch.empty((_lib.load().emage_bn_stats_workspace_bytes(rows, c) + 7) // 8, dtype=torch.float64, device=DEV)
        tag = f"bn[m{m} c{c}]"
        # one launch set
        dxb, gb, bb = _nans(m + 2, c + 4), _nans(c + 6), _nans(c + 6)
        ops._bn_backward(xd, mean_d, var_d, gd, eps, dyd, dxb[1:1 + m, 2:2 + c], gb[3:3 + c], bb[3:3 + c], ws(m))
        # the split form on all rows (count = M)
        sb, sdb, dxb2 = _nans(c + 6), _nans(c + 6), _nans(m + 2, c + 4)
        ops._bn_backward_sums(xd, mean_d, var_d, eps, dyd, sb[3:3 + c], sdb[3:3 + c], ws(m))
        ops._bn_backward_apply(xd, mean_d, var_d, gd, eps, dyd, sb[3:3 + c], sdb[3:3 + c], m, dxb2[1:1 + m, 2:2 + c])
        torch.cuda.synchronize()
        for nm, buf in (("dx", dxb), ("dx (split)", dxb2)):
            _nan_outside(f"{tag}.{nm}", buf, slice(1, 1 + m), slice(2, 2 + c))
            _cmp(f"{tag}.{nm}", buf[1:1 + m, 2:2 + c], dx_r, tdx)
        for nm, buf, rf, tol in (("dgamma", gb, dg_r, tdg), ("dbeta", bb, db_r, tdb), ("sum dy xhat", sb, dg_r, tdg), ("sum dy", sdb, db_r, tdb)):
            _nan_outside(f"{tag}.{nm}", buf, slice(3, 3 + c))
            _cmp(f"{tag}.{nm}", buf[3:3 + c], rf, tol)
        # emage_bn_backward IS its two halves with count = M (the same launches): the same bits
        assert torch.equal(dxb[1:1 + m, 2:2 + c], dxb2[1:1 + m, 2:2 + c]), f"{tag}: dx of the one-call form differs from the split form with count = M"
        assert torch.equal(gb[3:3 + c], sb[3:3 + c]) and torch.equal(bb[3:3 + c], sdb[3:3 + c]), f"{tag}: dgamma / dbeta differ from the two sums"
        # two shards with global statistics and the global count
        m1 = m // 2 + 1 if m > 2 else 1
        shards = [(0, m1), (m1, m)]
        sums = []
        for r0, r1 in shards:
            sdx, sd = ops.bn_backward_sums(xd[r0:r1], (mean_d, var_d), dyd[r0:r1], eps)
            sums.append((sdx.double().cpu(), sd.double().cpu()))
        tot = tuple((sums[0][i] + sums[1][i]).float().to(DEV) for i in range(2))
        dxs = _nans(m + 2, c + 4)
        wrong = []
        for r0, r1 in shards:
            ops._bn_backward_apply(xd[r0:r1], mean_d, var_d, gd, eps, dyd[r0:r1], tot[0], tot[1], m, dxs[1 + r0:1 + r1, 2:2 + c])
            wrong.append(ops.bn_backward_apply(xd[r0:r1], (mean_d, var_d), gd, dyd[r0:r1], tot, r1 - r0, eps))
        torch.cuda.synchronize()
        _nan_outside(f"{tag}.dx (two shards)", dxs, slice(1, 1 + m), slice(2, 2 + c))
        _cmp(f"{tag}.dx (two shards, count = {m})", dxs[1:1 + m, 2:2 + c], dx_r, tdx)
        _far(f"{tag}.dx vs count = shard rows", dxs[1:1 + m, 2:2 + c], torch.cat(wrong).cpu(), tdx)


# ---------------------------------------------------------------------------------------------------------------------------------
# convolution pieces: im2col_t_h2 (the W operand of the H2 weight-gradient contraction) and col2im (its adjoint: the input gradient)
# ---------------------------------------------------------------------------------------------------------------------------------

CONV_CASES = [
    # c, taps, stride, pad, lin, nseq        (lout = (lin + 2 pad - taps) // stride + 1; nseq * lout is never a multiple of 64)
    (1, 15, 5, 1600, 5000, 2),          # the waveform input of the first WavEncoder block (C = 1)
    (64, 15, 6, 0, 1638, 2),            # a stride-6 block
    (64, 15, 1, 7, 271, 3),             # a stride-1 conv2
    (128, 15, 3, 0, 134, 3),            # the stride-3 last block
    (256, 3, 1, 1, 37, 3),              # the taps-3 pad-1 convolutions
    (37, 5, 2, 2, 61, 3),               # stride > 1 with pad > 0, ragged C
]
CONV_IDS = [f"c{c}_k{k}_s{s}_p{p}" for c, k, s, p, _l, _n in CONV_CASES]


def _im2col(x, c, taps, stride, pad, lin, lout, nseq, flip=False):
    """(nseq * lin, c) channels-last rows -> (nseq * lout, taps * c), [seq * lout + l][tap * c + ch] = x[seq][l stride - pad + tap][ch]
    (0 outside the sequence); torch indexing only (differentiable).  flip: the taps in reverse order (the wrong variant)."""
    xp = tf.pad(x.reshape(nseq, lin, c), (0, 0, pad, pad))
    u = xp.unfold(1, taps, stride)[:, :lout]                              # (nseq, lout, c, taps)
    if flip:
        u = u.flip(-1)
    return u.permute(0, 1, 3, 2).reshape(nseq * lout, taps * c)


def _conv_input(c, lin, nseq, seed):
    g = _g(seed)
    xb = torch.randn(nseq * lin, c + 3, generator=g)
    return xb, xb[:, 1:1 + c]                                              # row-strided (C = 1: ldx = 4)


@pytest.mark.parametrize("case", CONV_CASES, ids=CONV_IDS)
def test_im2col_t_h2(case):
    """The H2 image of the transposed im2col matrix is bit for bit ops.h2_pack of the float32 im2col built by torch indexing, and its
    padding columns [M, mp) are zeros although the buffer was filled with NaN (the wrapper allocates with torch.empty).  Wrong reference:
    the taps in reverse order."""
    c, taps, stride, pad, lin, nseq = case
    lout = (lin + 2 * pad - taps) // stride + 1
    m = nseq * lout
    mp = ops.round_up(m, 64)
    assert m % 64
    xb, x = _conv_input(c, lin, nseq, seed=taps * 100 + c)
    col = torch.zeros(taps * c, mp)
    col[:, :m] = _im2col(x, c, taps, stride, pad, lin, lout, nseq).t()
    want = ops.h2_pack(col)
    buf = _nans(taps * c + 2, mp + 24)                                     # ld % 8 == 0, rows 16-byte aligned
    ops._im2col_t_h2(xb.to(DEV)[:, 1:1 + c], c, taps, stride, pad, lin, lout, nseq, buf[:taps * c, :mp])
    torch.cuda.synchronize()
    _nan_outside("im2col_t_h2", buf, slice(0, taps * c), slice(0, mp))
    got = buf[:taps * c, :mp].cpu()
    same = got.view(torch.int32) == want.view(torch.int32)
    assert bool(same.all()), f"im2col_t_h2 {case}: {int((~same).sum())} of {same.numel()} words differ from h2_pack(im2col)"
    assert bool((ops.h2_unpack(got)[:, m:] == 0).all())
    print(f"im2col_t_h2 {case}: bit-identical ({got.numel()} words, {taps * c * (mp - m)} padding zeros)")
    wrong = torch.zeros(taps * c, mp)
    wrong[:, :m] = _im2col(x, c, taps, stride, pad, lin, lout, nseq, flip=True).t()
    _far("im2col_t_h2 vs reversed taps", ops.h2_unpack(got), wrong, 1e-5 * _scale(col))


# col2im: every dx entry adds at most ceil(taps / stride) fp32 values: ~15 roundings of partial sums, a few 1e-7 of the scale.
COL2IM_TOL = 1e-5


@pytest.mark.parametrize("case", CONV_CASES, ids=CONV_IDS)
def test_col2im(case):
    """col2im against torch.autograd.grad in float64 of (im2col(x) * dcol).sum() with respect to x; dcol row-strided, dx into a NaN
    window.  Wrong reference: the taps in reverse order."""
    c, taps, stride, pad, lin, nseq = case
    lout = (lin + 2 * pad - taps) // stride + 1
    m = nseq * lout
    g = _g(taps * 1000 + c)
    dcb = torch.randn(m, taps * c + 4, generator=g)
    dcol = dcb[:, 2:2 + taps * c]
    x64 = torch.zeros(nseq * lin, c, dtype=torch.float64, requires_grad=True)
    ref, = torch.autograd.grad((_im2col(x64, c, taps, stride, pad, lin, lout, nseq) * dcol.double()).sum(), x64)
    x64w = torch.zeros(nseq * lin, c, dtype=torch.float64, requires_grad=True)
    wrong, = torch.autograd.grad((_im2col(x64w, c, taps, stride, pad, lin, lout, nseq, flip=True) * dcol.double()).sum(), x64w)
    buf = _nans(nseq * lin + 2, c + 3)
    ops._col2im(dcb.to(DEV)[:, 2:2 + taps * c], c, taps, stride, pad, lin, lout, nseq, buf[1:1 + nseq * lin, 1:1 + c])
    torch.cuda.synchronize()
    _nan_outside("col2im", buf, slice(1, 1 + nseq * lin), slice(1, 1 + c))
    got = buf[1:1 + nseq * lin, 1:1 + c]
    tol = COL2IM_TOL * _scale(ref)
    _cmp(f"col2im {case}", got, ref, tol)
    _far("col2im vs reversed taps", got, wrong, tol)


# ---------------------------------------------------------------------------------------------------------------------------------
# first WavEncoder layer: dW of conv1d(wav, W, stride, padding) (Cin = 1)
# ---------------------------------------------------------------------------------------------------------------------------------

# float64 sums of fp32 products: each product rounded once (2^-24 relative), the sums exact to ~1e-16: far below 1e-5 of the scale.
WAV_TOL = 1e-5
WAV_CASES = [
    # b, samples, c, taps, stride, pad
    (1, 5000, 128, 15, 5, 1600),
    (3, 5000, 128, 15, 5, 1600),        # M = 3 x 1638: not a multiple of the 1024-row chunk
    (1, 136000, 128, 15, 5, 1600),      # one long wave: 27 838 rows
    (2, 3001, 64, 15, 5, 1600),
]


@pytest.mark.parametrize("case", WAV_CASES, ids=[f"b{b}_l{l}_c{c}" for b, l, c, *_ in WAV_CASES])
def test_wav_conv_in_backward(case):
    """The weight gradient (C, taps) of the first WavEncoder layer against float64 autograd of conv1d(wav, W, stride, padding) with
    respect to W; dy and the waveform as strided views.  Wrong reference: the taps in reverse order."""
    b, length, c, taps, stride, pad = case
    lout = (length + 2 * pad - taps) // stride + 1
    m = b * lout
    g = _g(length + c + b)
    wavb = torch.randn(b, length + 7, generator=g)
    dyb = torch.randn(m, c + 4, generator=g)
    wav, dy = wavb[:, :length], dyb[:, 2:2 + c]
    w64 = torch.zeros(c, 1, taps, dtype=torch.float64, requires_grad=True)
    y = tf.conv1d(wav.double().unsqueeze(1), w64, stride=stride, padding=pad)             # (b, c, lout)
    assert y.shape[-1] == lout
    ref, = torch.autograd.grad(y, w64, dy.double().view(b, lout, c).permute(0, 2, 1))
    ref = ref[:, 0]
    buf = _nans(c * taps + 16)
    nbytes = _lib.load().emage_wav_conv_in_backward_workspace_bytes(m, c, taps)
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=DEV)
    ops._wav_conv_in_backward(dyb.to(DEV)[:, 2:2 + c], wavb.to(DEV)[:, :length], lout, taps, stride, pad, buf[:c * taps].view(c, taps), ws)
    torch.cuda.synchronize()
    _nan_outside("wav_conv_in_backward", buf, slice(0, c * taps))
    got = buf[:c * taps].view(c, taps)
    tol = WAV_TOL * _scale(ref)
    _cmp(f"wav_conv_in_backward {case}", got, ref, tol)
    _far("wav_conv_in_backward vs reversed taps", got, ref.flip(-1), tol)


# ---------------------------------------------------------------------------------------------------------------------------------
# loss gradients: weight * nll_loss(log_softmax(logits), index) and weight * mse_loss(pred, target), mean over the batch
# ---------------------------------------------------------------------------------------------------------------------------------

# nll: scale (softmax - onehot) with an fp32 max, fp32 exp and an fp32 sum of K terms: the entries that matter (within ~20 of the row max)
# carry a few ulp; 1e-5 of the scale.  mse: scale (pred - target), three roundings: 4 x 2^-24 of the scale.
NLL_TOL, MSE_TOL = 1e-5, 4 * EPS32


@pytest.mark.parametrize("k", [1, 63, 64, 65, 256, 1000])
def test_loss_gradients(k):
    """nll_loss_grad with logits spread over +-80, one row with a +1e4 outlier and one with a -1e4 outlier (the max subtraction),
    targets at 0 and K - 1, strided logits; mse_loss_grad on strided operands.  Wrong references: the target one class off (K > 1),
    the factor 2 of the squared error left out."""
    m, weight = 37, 0.7
    g = _g(k)
    lb = (torch.rand(m, k + 3, generator=g) * 2.0 - 1.0) * 80.0
    lb[5, 1 + (k - 1) // 2] = 1e4
    lb[6, 1 + k // 3] = -1e4
    logits = lb[:, 1:1 + k]
    idx = torch.randint(0, k, (m,), generator=g)
    idx[0], idx[1] = 0, k - 1
    idx[5] = (k - 1) // 2
    xd = logits.double().requires_grad_()
    ref, = torch.autograd.grad(weight * tf.nll_loss(torch.log_softmax(xd, dim=1), idx), xd)
    buf = _nans(m + 2, k + 5)
    ops._nll_loss_grad(lb.to(DEV)[:, 1:1 + k], idx.to(DEV), weight, buf[1:1 + m, 2:2 + k])
    torch.cuda.synchronize()
    _nan_outside("nll_loss_grad", buf, slice(1, 1 + m), slice(2, 2 + k))
    got = buf[1:1 + m, 2:2 + k]
    tol = NLL_TOL * max(_scale(ref), weight / m)
    _cmp(f"nll_loss_grad k{k}", got, ref, tol)
    if k > 1:
        xw = logits.double().requires_grad_()
        wrong, = torch.autograd.grad(weight * tf.nll_loss(torch.log_softmax(xw, dim=1), (idx + 1) % k), xw)
        _far("nll_loss_grad vs target one class off", got, wrong, tol)

    pb, tb = torch.randn(m, k + 2, generator=g) * 3.0, torch.randn(m + 1, k + 4, generator=g)
    pred, target = pb[:, 1:1 + k], tb[1:, 3:3 + k]
    pd = pred.double().requires_grad_()
    ref, = torch.autograd.grad(weight * tf.mse_loss(pd, target.double()), pd)
    buf = _nans(m + 2, k + 5)
    ops._mse_loss_grad(pb.to(DEV)[:, 1:1 + k], tb.to(DEV)[1:, 3:3 + k], weight, buf[1:1 + m, 2:2 + k])
    torch.cuda.synchronize()
    _nan_outside("mse_loss_grad", buf, slice(1, 1 + m), slice(2, 2 + k))
    got = buf[1:1 + m, 2:2 + k]
    tol = MSE_TOL * _scale(ref)
    _cmp(f"mse_loss_grad k{k}", got, ref, tol)
    _far("mse_loss_grad vs the factor 2 left out", got, ref / 2, tol)
