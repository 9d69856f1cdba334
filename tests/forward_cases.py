"""The case table of the forward-kernel tests: for every operation the seeded input builders, the float64 reference (plain torch on
the CPU of the mathematical operation; rotations through the dtype-generic functions of oracle/emage_oracle.py called with float64
tensors), the tolerance derived from the kernel's arithmetic (stated next to each case) and one plausible WRONG reference per feature.

Every `check_*` takes `impl`: `pantomatrix_amd.ops` (the HIP kernels, tensors on the device: tests/test_forward_kernels_gpu.py) or
`tests/fake_ops.py` (fp32 torch on the CPU: tests/test_forward_kernels_host.py, which proves that a correct fp32 implementation passes
every tolerance and that every wrong reference is rejected).  Conventions as in test_backward_kernels_gpu.py: outputs are views of NaN-filled
buffers that must still be NaN outside the block; every comparison prints its max error; a wrong reference must miss by more than FAR x the
tolerance.  Hyper-parameters that cross the C ABI as `float` (eps, momentum, betas, lr, dt ...) enter the float64 reference with their
fp32-rounded value: that value is the kernel's input."""
import functools
import math

import torch

from kernel_checks import EPS32, FAR, _cmp, _far, _nan_outside
from oracle import emage_oracle as orc
from pantomatrix_amd import ops
from pantomatrix_amd._lib import BF16, F32, H2

EPS64_SUB = 2.0 ** -50      # the float64 subtraction  E[x^2] - mean^2  of the chunked variance


def gen(seed):
    return torch.Generator().manual_seed(seed)


def dev_of(impl):
    return "cuda" if impl is ops else "cpu"


def nans(dev, *shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def f32(v):
    """The value a `float` argument of the C ABI carries."""
    return float(torch.tensor(v, dtype=torch.float32))


def far(name, got, wrong, tol):
    """`_far` with a NaN in the wrong reference counted as an infinite miss."""
    _far(name, got, torch.nan_to_num(wrong.detach().double().cpu(), nan=1e30), tol)


def bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    view = torch.int16 if a.dtype == torch.bfloat16 else torch.int32 if a.dtype == torch.float32 else torch.int64
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(view), b.view(view))


# ---------------------------------------------------------------------------------------------------------------------------------
# LayerNorm forward (elementwise.hip / ln_row.h): one wave per row, 4 rows per block, C % 64 == 0, C <= 1024
# ---------------------------------------------------------------------------------------------------------------------------------
LN_C = (64, 320, 768, 1024)        # 16 active lanes | 2 register groups, the second partly filled | the model width | every group live
LN_M = (1, 3, 5, 130)              # less than a block, a ragged last block, many blocks
LN_DTYPES = {"f32": F32, "bf16": BF16, "h2": H2}
LN_CONST = 2.5                     # <= 13 significant bits: every partial sum of <= 1024 copies is exact in fp32, so mean == the value
LN_EPS = f32(1e-5)


def ln_inputs(m, c, dtype, seed):
    """Row kinds by (row + m) % 4: 0 N(0,1) | 1 mean 1e3, unit spread | 2 constant | 3 N(0,1) with one 1e4 outlier."""
    g = gen(seed)
    x = torch.randn(m, c, generator=g)
    kind = (torch.arange(m) + m) % 4
    x[kind == 1] += 1e3
    x[kind == 2] = LN_CONST
    r3 = (kind == 3).nonzero().flatten()
    x[r3, (r3 * 37 + 11) % c] = 1e4
    gamma, beta = 1 + 0.5 * torch.randn(c, generator=g), torch.randn(c, generator=g)
    add = torch.randn(m, c, generator=g)
    td = torch.bfloat16 if dtype == BF16 else torch.float32
    return x.to(td), gamma, beta, add.to(td), kind


def ln_ref(x, gamma, beta, add, unbiased=False):
    """float64 LayerNorm of the stored row.  tol per entry: 8 EPS32 (max|row| rstd |gamma| + |ref|) — the row mean is an fp32 sum of C terms
    (error ~ EPS32 max|row|, amplified by rstd |gamma|), the affine chain adds a few EPS32 |ref| — and never above 1e-4 of the output's scale.
    With a residual, |ref| is the larger of the result and of xhat gamma + beta, the fp32 intermediate the residual is added to: where the
    residual cancels it, the intermediate's rounding is what is left (torch's own layer_norm + add misses the plain formula there)."""
    xd, c = x.double(), x.shape[1]
    mean = xd.mean(1, keepdim=True)
    var = ((xd - mean) ** 2).sum(1, keepdim=True) / (c - 1 if unbiased else c)
    rstd = 1.0 / torch.sqrt(var + LN_EPS)
    ref = (xd - mean) * rstd * gamma.double() + beta.double()
    mag = ref.abs()
    if add is not None:
        ref = ref + add.double()
        mag = torch.maximum(mag, ref.abs())
    tol = 8 * EPS32 * (xd.abs().amax(1, keepdim=True) * rstd * gamma.double().abs() + mag)
    return ref, torch.minimum(tol, 1e-4 * ref.abs().max())


def check_layernorm(impl, name, c):
    dev, dtype = dev_of(impl), LN_DTYPES[name]
    ld = c + 64
    for m in LN_M:
        for with_add in (False, True):
            x, gamma, beta, add, kind = ln_inputs(m, c, dtype, seed=1000 * c + 10 * m + with_add)
            xb, ab = nans(dev, m + 2, ld, dtype=x.dtype), nans(dev, m + 2, ld, dtype=x.dtype)
            xb[1:m + 1, :c], ab[1:m + 1, 64:] = x.to(dev), add.to(dev)
            xv, av = xb[1:m + 1, :c], (ab[1:m + 1, 64:] if with_add else None)
            gd, bd = gamma.to(dev), beta.to(dev)
            yfb = nans(dev, m + 2, ld)
            yb = nans(dev, m + 2, ld, dtype=x.dtype)
            blk = (slice(1, m + 1), slice(32, 32 + c))
            impl.layernorm(dtype, xv, gd, bd, LN_EPS, av, yfb[blk], yb[blk])
            tag = f"layernorm[{name} M={m} C={c}{' +add' if with_add else ''}]"
            _nan_outside(tag + ".y_f32", yfb, *blk)
            _nan_outside(tag + ".y", yb, *blk)
            yf, y = yfb[blk].cpu(), yb[blk].cpu()
            ref, tol = ln_ref(x, gamma, beta, add if with_add else None)
            _cmp(tag, yf, ref, tol)
            # a constant row: v - mean is exactly 0, so the output is exactly beta (+ add)
            want = beta.expand(m, c) + add.float() if with_add else beta.expand(m, c)
            assert torch.equal(yf[kind == 2], want[kind == 2]), tag + ": constant rows must give exactly beta (+ add)"
            if dtype == F32:
                assert bits_equal(y, yf), tag + ": y vs y_f32"
            elif dtype == BF16:          # f32_to_bf16 (common.h) adds 0x7fff + the lowest kept bit: round to nearest, ties to even = torch's cast
                assert bits_equal(y, yf.to(torch.bfloat16)), tag + ": y is not round-to-nearest-even of the kernel's own y_f32"
            else:
                assert bits_equal(y, impl.h2_cast(yfb[blk], c, 1.0).cpu()), tag + ": the H2 image is not h2_cast of the kernel's own y_f32"
                y32 = nans(dev, m + 2, ld)
                impl.layernorm(F32, xv, gd, bd, LN_EPS, av, y32[blk], None)
                assert bits_equal(y32[blk], yf), tag + ": y_f32 of the H2 call vs the F32 call"
            # wrong references: unbiased variance (on the N(0,1) rows, whose tolerance is the tightest); the residual left out
            r0 = kind == 0
            if bool(r0.any()):
                far(tag + " vs unbiased variance", yf[r0], ln_ref(x, gamma, beta, add if with_add else None, unbiased=True)[0][r0], tol[r0])
            if with_add:
                far(tag + " vs no residual", yf, ln_ref(x, gamma, beta, None)[0], tol)


LN_REFUSED = {"C=96": (96, 96 + 64), "C=1088": (1088, 1088 + 64), "ldx=C+2": (768, 768 + 2)}


def layernorm_refused_args(dev, which):
    """(x, gamma, beta, y) the kernel must refuse: C not a multiple of 64, C above 1024, a row pitch that breaks the 16-byte row alignment."""
    c, ld = LN_REFUSED[which]
    buf = torch.zeros(4, ld, device=dev)
    return buf[:, :c], torch.ones(c, device=dev), torch.zeros(c, device=dev), torch.zeros(4, c + 64, device=dev)[:, :c]      # y: an aligned pitch


# ---------------------------------------------------------------------------------------------------------------------------------
# BatchNorm statistics (train.hip, col_reduce.h): float64 chunk partials (stat_rows(M) rows each), finalize over 16 lanes
# ---------------------------------------------------------------------------------------------------------------------------------
BN_M = (1, 2, 63, 64, 65, 257, 1025, 33001)     # 33 001: 68 rows per chunk (> STAT_CHUNK), 486 chunks, 31 per finalize lane
BN_CONST, BN_CONST_FULL = 2.5, 1000.1           # short mantissa: M v^2 is exact in float64 -> variance exactly 0; full mantissa: only up to the subtraction


def bn_cs(m):
    return (1, 63, 64) + ((65,) if m == 33001 else ())


def bn_stats_inputs(m, c, seed):
    """Channel kinds by (c + m) % 4: 0 N(0,1) | 1 mean 1e3, std 1e-2 | 2 constant 2.5 | 3 constant 1000.1; x a column slice of a wider buffer."""
    g = gen(seed)
    xb = torch.randn(m, c + 5, generator=g)
    kind = (torch.arange(c) + m) % 4
    x = xb[:, 2:2 + c]
    x[:, kind == 1] = 1e3 + 1e-2 * x[:, kind == 1]
    x[:, kind == 2] = BN_CONST
    x[:, kind == 3] = BN_CONST_FULL
    rm, rv = torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5
    return xb, kind, rm, rv


def check_bn_stats(impl, m):
    dev = dev_of(impl)
    for c in bn_cs(m):
        xb, kind, rm0, rv0 = bn_stats_inputs(m, c, seed=7 * m + c)
        xd = xb[:, 2:2 + c].double()
        mean = xd.mean(0)
        var = ((xd - mean) ** 2).mean(0)
        # float64 sums, one rounding to fp32: a few EPS32 of the result; the variance also carries the float64 subtraction E[x^2] - mean^2
        tol_mean = 2 * EPS32 * mean.abs() + 2.0 ** -45 * xd.abs().mean(0)
        tol_var = 4 * EPS32 * var + EPS64_SUB * (mean ** 2 + var)
        x = xb.to(dev)[:, 2:2 + c]
        for mom in (None, 0.0, 0.1, 1.0):
            tag = f"bn_stats[M={m} C={c} momentum={mom}]"
            rm, rv = (None, None) if mom is None else (rm0.clone().to(dev), rv0.clone().to(dev))
            got_mean, got_var = impl.bn_stats(x, rm, rv, 0.1 if mom is None else mom)
            _cmp(tag + ".mean", got_mean, mean, tol_mean)
            _cmp(tag + ".var", got_var, var, tol_var)
            gv = got_var.cpu()
            assert bool((gv >= 0).all()), tag + ": negative variance"
            assert bool((gv[kind == 2] == 0).all()) and bool((got_mean.cpu()[kind == 2] == BN_CONST).all()), tag + ": constant channel"
            if m == 1:
                assert bool((gv == 0).all()), tag + ": one row has variance 0"
            if m > 1 and bool((kind == 0).any()):
                far(tag + ".var vs unbiased variance", got_var[kind == 0], var[kind == 0] * m / (m - 1), tol_var[kind == 0])
            if mom is None:
                continue
            mo = f32(mom)
            unb = var * m / max(m - 1, 1)
            ref_rm = (1 - mo) * rm0.double() + mo * mean
            ref_rv = (1 - mo) * rv0.double() + mo * unb
            # (1 - momentum) * running + momentum * fp32(statistic): in fp32 two products and a sum, <= 3 roundings at the magnitude of the two
            # terms (they may cancel) -> 4 EPS32 of them, plus the statistic's own tolerance
            tol_rm = 4 * EPS32 * ((1 - mo) * rm0.double().abs() + mo * mean.abs()) + mo * tol_mean
            tol_rv = 4 * EPS32 * ((1 - mo) * rv0.double() + mo * unb) + mo * (tol_var + EPS32 * var) * m / max(m - 1, 1)
            assert bool(torch.isfinite(rv.cpu()).all()), tag + ": running_var not finite"
            _cmp(tag + ".running_mean", rm, ref_rm, tol_rm)
            _cmp(tag + ".running_var", rv, ref_rv, tol_rv)
            if mo > 0 and 1 < m < 2000 and bool((kind == 0).any()):
                far(tag + ".running_var vs biased variance", rv[kind == 0], ((1 - mo) * rv0.double() + mo * var)[kind == 0], tol_rv[kind == 0])


# ---------------------------------------------------------------------------------------------------------------------------------
# BatchNorm apply: out = leaky(bn(x) + shortcut); grid_for caps at 8192 blocks of 256
# ---------------------------------------------------------------------------------------------------------------------------------
BN_APPLY_CASES = [(m, c, mode, slope) for (m, c) in ((1, 1), (130, 65)) for mode in ("none", "raw", "bn") for slope in (0.2, 1.0)] \
    + [(8200, 257, "bn", 0.2)]                  # 2 107 400 elements > 8192 * 256: the grid-stride loop runs a second time
BN_EPS = f32(1e-5)


def check_bn_apply(impl, m, c, mode, slope):
    dev = dev_of(impl)
    g = gen(100 * m + c + len(mode))
    xb, sb = torch.randn(m, c + 3, generator=g), torch.randn(m, c + 7, generator=g)
    p = [torch.randn(c, generator=g) for _ in range(2)] + [torch.rand(c, generator=g) * 1.5 + 0.5 for _ in range(2)]      # means, variances
    mean, sc_mean, var, sc_var = p
    gamma, beta, sc_gamma, sc_beta = (torch.randn(c, generator=g) for _ in range(4))
    sl = f32(slope)

    def ref(slope=sl, mode=mode, rsqrt=True, sc_own_stats=True):
        """tol per entry: 8 EPS32 (|xhat gamma| + |beta| + the same of the shortcut + |ref|): the chain (x - mean) * invstd * gamma + beta
        (+ r), leaky — about 7 roundings on the product, 3 on the sums."""
        def bn(v, mu, vr, ga, be):
            xh = (v.double() - mu.double()) / (torch.sqrt(vr.double() + BN_EPS) if rsqrt else vr.double() + BN_EPS) * ga.double()
            return xh + be.double(), xh.abs() + be.double().abs()
        v, mag = bn(xb[:, 1:1 + c], mean, var, gamma, beta)
        if mode == "raw":
            v, mag = v + sb[:, 4:4 + c].double(), mag + sb[:, 4:4 + c].double().abs()
        elif mode == "bn":
            r, rmag = bn(sb[:, 4:4 + c], *((sc_mean, sc_var) if sc_own_stats else (mean, var)), sc_gamma, sc_beta)
            v, mag = v + r, mag + rmag
        out = torch.where(v > 0, v, v * slope)
        return out, 8 * EPS32 * (mag + out.abs())

    d = lambda t: t.to(dev)
    x, sc = d(xb)[:, 1:1 + c], d(sb)[:, 4:4 + c]
    ob = nans(dev, m + 2, c + 9)
    blk = (slice(1, m + 1), slice(5, 5 + c))
    impl.bn_apply(x, (d(mean), d(var)), d(gamma), d(beta), ob[blk], slope=slope, sc=None if mode == "none" else sc,
                  sc_bn=(d(sc_mean), d(sc_var), d(sc_gamma), d(sc_beta)) if mode == "bn" else None, eps=BN_EPS)
    tag = f"bn_apply[{m}x{c} {mode} slope={slope}]"
    _nan_outside(tag, ob, *blk)
    want, tol = ref()
    _cmp(tag, ob[blk], want, tol)
    far(tag + " vs var in place of sqrt(var)", ob[blk], ref(rsqrt=False)[0], tol)
    if slope != 1.0 and bool((ref(slope=1.0)[0] < 0).any()):
        far(tag + " vs no LeakyReLU", ob[blk], ref(slope=1.0)[0], tol)
    if mode != "none":
        far(tag + " vs no shortcut", ob[blk], ref(mode="none")[0], tol)
    if mode == "bn":
        far(tag + " vs shortcut normalised with the main statistics", ob[blk], ref(sc_own_stats=False)[0], tol)


# ---------------------------------------------------------------------------------------------------------------------------------
# losses: block partials in float64; at most 1023 blocks of 256 threads, grid-stride above 261 888 elements (mse) / rows (nll)
# ---------------------------------------------------------------------------------------------------------------------------------
MSE_SHAPES = [(1, 1), (5, 51), (1, 257), (1023, 256), (1030, 255)]          # M C = 1, 255, 257, 261 888, 262 650
NLL_SHAPES = [(130, k) for k in (1, 2, 37, 256, 1000)] + [(261888, 3), (262145, 3)]
LOSS0, LOSS_WEIGHTS = 1.25, (3.0, 0.5)
LOSS_CAP = 1023 * 256


def check_mse_loss(impl, m, c):
    dev = dev_of(impl)
    g = gen(31 * m + c)
    pb, t = torch.randn(m, c + 3, generator=g), torch.randn(m, c, generator=g)
    pred = pb.to(dev)[:, 2:2 + c]
    loss, ws = torch.full((1,), LOSS0, dtype=torch.float64, device=dev), impl.loss_workspace(dev)
    for w in LOSS_WEIGHTS:
        impl.mse_loss(pred, t.to(dev), w, loss, ws)
    d2 = (pb[:, 2:2 + c].double() - t.double()) ** 2
    wsum = sum(LOSS_WEIGHTS)
    ref = torch.tensor([LOSS0 + wsum * float(d2.mean())], dtype=torch.float64)
    # per term fl(fl(a - b)^2): 3 roundings, relative 3 EPS32 of the term; the sum and the scalar are float64
    tol = 4 * EPS32 * wsum * float(d2.mean()) + 2.0 ** -40 * float(ref.abs())
    tag = f"mse_loss[{m}x{c}]"
    _cmp(tag, loss, ref, tol)
    far(tag + " vs '=' in place of '+='", loss, ref - LOSS0, tol)
    if m * c > LOSS_CAP:
        far(tag + " vs no grid stride", loss, torch.tensor([LOSS0 + wsum * float(d2.reshape(-1)[:LOSS_CAP].sum()) / (m * c)]), tol)
    return loss, ws


def nll_inputs(m, k):
    g = gen(17 * m + k)
    lb = (torch.rand(m, k + 3, generator=g) * 2 - 1) * 80.0              # +-80: expf(x - max) underflows for most classes
    return lb, torch.randint(0, k, (m,), generator=g)


def check_nll_loss(impl, m, k):
    dev = dev_of(impl)
    lb, index = nll_inputs(m, k)
    logits = lb.to(dev)[:, 1:1 + k]
    loss, ws = torch.full((1,), LOSS0, dtype=torch.float64, device=dev), impl.loss_workspace(dev)
    for w in LOSS_WEIGHTS:
        impl.nll_loss(logits, index.to(dev), w, loss, ws)
    impl.loss_check(ws)                                                   # every index in range: the flag stays clear
    xd = lb[:, 1:1 + k].double()
    mx, lse = xd.amax(1), torch.logsumexp(xd, 1)
    xt = xd.gather(1, index.view(-1, 1)).flatten()
    rows = lse - xt
    wsum = sum(LOSS_WEIGHTS)
    ref = torch.tensor([LOSS0 + wsum * float(rows.mean())], dtype=torch.float64)
    # per row EPS32 (4 (|x_t| + |max| + |lse - max|) + K): two subtractions at the logits' magnitude, logf of an fp32 sum of K terms in [0, 1]
    tol_rows = EPS32 * (4 * (xt.abs() + mx.abs() + (lse - mx).abs()) + k)
    tol = wsum * float(tol_rows.mean()) + 2.0 ** -40 * float(ref.abs())
    tag = f"nll_loss[{m}x{k}]"
    _cmp(tag, loss, ref, tol)
    far(tag + " vs '=' in place of '+='", loss, ref - LOSS0, tol)
    if k > 1:
        far(tag + " vs the max left in (log of the shifted sum only)", loss, torch.tensor([LOSS0 + wsum * float((lse - mx - xt).mean())]), tol)
    if m > LOSS_CAP:
        far(tag + " vs no grid stride", loss, torch.tensor([LOSS0 + wsum * float(rows[:LOSS_CAP].sum()) / m]), tol)
    return logits, index, loss, ws


# ---------------------------------------------------------------------------------------------------------------------------------
# col_sum: float64 chunk partials, finalize over 16 lanes (17 chunks at M = 1025 / 1089: trailing lanes own empty ranges)
# ---------------------------------------------------------------------------------------------------------------------------------
COLSUM_M = (1, 63, 64, 65, 1025, 1089, 33001)
COLSUM_C = (1, 15, 16, 17, 64, 65, 130)


def check_col_sum(impl, m):
    dev = dev_of(impl)
    for c in COLSUM_C:
        g = gen(13 * m + c)
        xb, yb = torch.randn(m, c + 3, generator=g) + 1.0, torch.randn(m, c + 6, generator=g)
        xb[-1], yb[-1] = 3.0, -2.0                                        # the last row is worth 3 (or 6) in every column: dropping it shows
        out0 = torch.randn(c, generator=g) * 10
        x, y = xb.to(dev)[:, 3:3 + c], yb.to(dev)[:, 1:1 + c]
        for with_y in (False, True):
            terms = xb[:, 3:3 + c].double() * (yb[:, 1:1 + c].double() if with_y else 1.0)
            s = terms.sum(0)
            for acc in (False, True):
                tag = f"col_sum[{m}x{c}{' *y' if with_y else ''}{' +=' if acc else ''}]"
                ref = out0.double() + s if acc else s
                # float64 sum of fp32 terms (x y rounded in fp32 first: EPS32 sum|terms|), rounded to fp32, then one fp32 add into `out`
                tol = 2 * EPS32 * (ref.abs() + s.abs()) + (EPS32 if with_y else 2.0 ** -45) * terms.abs().sum(0)
                ob = nans(dev, c + 4)
                ob[2:2 + c] = out0.to(dev)
                impl.col_sum(x, y if with_y else None, out=ob[2:2 + c], accumulate=acc)
                _nan_outside(tag, ob, slice(2, 2 + c))
                _cmp(tag, ob[2:2 + c], ref, tol)
                if m > 1:
                    far(tag + " vs last row dropped", ob[2:2 + c], ref - terms[-1], tol)
                elif with_y:
                    far(tag + " vs y ignored", ob[2:2 + c], ref - s + xb[:, 3:3 + c].double().sum(0), tol)
                if acc:
                    far(tag + " vs overwrite", ob[2:2 + c], s, tol)
                if impl is ops:          # the deferred multi-finalize launch: the same bits as the single launch
                    q, ob2 = ops.FinalizeQueue(), nans(dev, c + 4)
                    ob2[2:2 + c] = out0.to(dev)
                    ops.col_sum(x, y if with_y else None, out=ob2[2:2 + c], accumulate=acc, defer=q)
                    q.flush()
                    assert bits_equal(ob2, ob), tag + ": deferred finalize differs from the single launch"
                if not with_y and not acc and c == COLSUM_C[-1]:
                    _cmp(tag + " (out=None)", impl.col_sum(x), s, tol)


# ---------------------------------------------------------------------------------------------------------------------------------
# transpose (32 x 32 tiles through LDS) and mul_add (dropout mask stored (T, B), rows running (B, T)): exact
# ---------------------------------------------------------------------------------------------------------------------------------
TRANSPOSE_SIZES = (1, 31, 32, 33, 100)


def check_transpose(impl):
    dev = dev_of(impl)
    for m in TRANSPOSE_SIZES:
        for n in TRANSPOSE_SIZES:
            xb = torch.randn(m, n + 3, generator=gen(100 * m + n))
            ob = nans(dev, n + 2, m + 5)
            blk = (slice(1, n + 1), slice(2, 2 + m))
            impl.transpose(xb.to(dev)[:, 3:], ob[blk])
            tag = f"transpose[{m}x{n}]"
            _nan_outside(tag, ob, *blk)
            assert torch.equal(ob[blk].cpu(), xb[:, 3:].t()), tag
            if m > 1 and n > 1:
                assert not torch.equal(ob[blk].cpu(), xb[:, 3:].reshape(n, m)), tag + ": the data cannot tell a transpose from a copy"


MUL_ADD_CASES = [(b, t, c, res, swap) for (b, t, c) in ((3, 7, 40), (7, 3, 41)) for res in (False, True) for swap in (False, True)] \
    + [(8, 1025, 257, True, True)]              # 2 107 400 elements > 8192 * 256


def check_mul_add(impl, b, t, c, res, swap):
    dev = dev_of(impl)
    g = gen(1000 * b + 10 * t + c)
    m = b * t
    ab, rb = torch.randn(m, c + 3, generator=g), torch.randn(m, c + 1, generator=g)
    mask = (torch.rand(m, c, generator=g) >= 0.1).float() / f32(0.9)
    a, r = ab[:, 3:], rb[:, :c]
    mk = mask.view(t, b, c).transpose(0, 1).reshape(m, c) if swap else mask             # stream row (b, t) <-> mask row (t, b)
    want = a * mk + r if res else a * mk              # one fp32 multiply, one fp32 add, no contraction: the kernel's exact arithmetic
    ob = nans(dev, m + 1, c + 2)
    blk = (slice(0, m), slice(1, 1 + c))
    impl.mul_add(ab.to(dev)[:, 3:], mask.to(dev), rb.to(dev)[:, :c] if res else None, ob[blk], mask_t_rows=t if swap else 0)
    tag = f"mul_add[b={b} t={t} C={c}{' +res' if res else ''}{' (T,B) mask' if swap else ''}]"
    _nan_outside(tag, ob, *blk)
    assert torch.equal(ob[blk].cpu(), want), f"{tag}: max err {float((ob[blk].cpu() - want).abs().max()):.3e}"
    prod = a.double() * mk.double()
    _cmp(tag, ob[blk], prod + (r.double() if res else 0.0), 2 * EPS32 * (prod.abs() + want.abs().double()) + 1e-30)
    if swap:
        assert not torch.equal(ob[blk].cpu(), a * mask + r if res else a * mask), tag + ": the data cannot tell the row mappings apart"


# ---------------------------------------------------------------------------------------------------------------------------------
# Adam: three entry points against torch.optim.Adam in float64 from the same state
# ---------------------------------------------------------------------------------------------------------------------------------
ADAM_N = (1, 255, 4095, 4096, 4097, 10000)      # ADAM_CHUNK = 4096
ADAM_CASES = [(start, wd) for start in (1, 10000) for wd in (0.0, 0.01)]
ADAM_HP = dict(lr=f32(1.5e-4), beta1=f32(0.9), beta2=f32(0.999), eps=f32(1e-8))
ADAM_HP_EXACT = dict(lr=1.5e-4, beta1=0.9, beta2=0.999, eps=1e-8)      # what torch.optim.Adam(betas=(0.9, 0.999)) computes with in float64
ADAM_STEPS = 3


def adam_state(n, start, seed):
    """param, exp_avg, exp_avg_sq, and ADAM_STEPS gradients.  Entries 0 mod 5 have zero gradients; entries 1 mod 5 live where eps
    dominates (exp_avg_sq 1e-16, gradients and exp_avg ~1e-8).  start = 1: the moments start at zero, as torch's do."""
    g = gen(97 * n + start)
    p = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) for _ in range(ADAM_STEPS)]
    idx = torch.arange(n)
    for gr in grads:
        gr[idx % 5 == 0] = 0.0
        gr[idx % 5 == 1] *= 1e-8
    if start == 1:
        return p, torch.zeros(n), torch.zeros(n), grads
    m, v = 0.1 * torch.randn(n, generator=g), 0.01 * torch.rand(n, generator=g) + 1e-6
    m[idx % 5 == 1] *= 1e-7
    v[idx % 5 == 1] = 1e-16
    return p, m, v, grads


class HostAdamTable:
    """What `fake_ops.adam_multi` reads of an `ops.AdamTable`."""

    def __init__(self, quads, device):
        self.keep = quads


def adam_table(impl, quads, dev):
    return (ops.AdamTable if impl is ops else HostAdamTable)(quads, dev)


def adam_ref(p, m, v, grads, start, wd, grad_scale=1.0, bias_correction=True, hp=None):
    """torch.optim.Adam in float64 -> [(p, m, v, tol_p, tol_m, tol_v) after each step].  tol per entry: 8 EPS32 of the quantity's scale per
    step = the magnitudes of the terms it is built from, with |g| + wd |p| for the gradient (the terms may cancel):
        exp_avg     b1 |m| + (1 - b1) |g|          exp_avg_sq   b2 v + (1 - b2) |g|^2          param   |p|
    Errors carry over as the recurrences carry them (b1, b2 of the previous step's tolerance; the whole of the parameter's), and the
    parameter also takes the errors of both moments through its update  step_size m / (sqrt(v) / sqrt(1 - b2^t) + eps)."""
    hp = hp or ADAM_HP
    b1, b2, wdf = hp["beta1"], hp["beta2"], f32(wd)
    pp = p.double().clone().requires_grad_()
    opt = torch.optim.Adam([pp], lr=hp["lr"], betas=(b1, b2), eps=hp["eps"], weight_decay=wdf)
    opt.state[pp] = dict(step=torch.tensor(float(start - 1 if bias_correction else 10 ** 6)), exp_avg=m.double().clone(), exp_avg_sq=v.double().clone())
    out = []
    tol_p, tol_m, tol_v = (torch.zeros_like(pp.detach()) for _ in range(3))
    for gr in grads:
        st = opt.state[pp]
        m_old, v_old, p_old = st["exp_avg"].clone(), st["exp_avg_sq"].clone(), pp.detach().clone()
        pp.grad = gr.double() * grad_scale
        gmag = pp.grad.abs() + wdf * p_old.abs()
        opt.step()
        st = opt.state[pp]
        t = float(st["step"])
        tol_m = b1 * tol_m + 8 * EPS32 * (b1 * m_old.abs() + (1 - b1) * gmag)
        tol_v = b2 * tol_v + 8 * EPS32 * (b2 * v_old + (1 - b2) * gmag ** 2)
        root = st["exp_avg_sq"].sqrt() / math.sqrt(1 - b2 ** t)
        step_size = hp["lr"] / (1 - b1 ** t)
        d_root = tol_v / (2 * st["exp_avg_sq"].sqrt() * math.sqrt(1 - b2 ** t) + 1e-300)                 # d sqrt(v) = dv / (2 sqrt(v))
        upd = step_size * st["exp_avg"].abs() / (root + hp["eps"])
        tol_p = tol_p + 8 * EPS32 * (p_old.abs() + upd) + step_size * tol_m / (root + hp["eps"]) + upd * torch.clamp(d_root / (root + hp["eps"]), max=1.0)
        out.append((pp.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), tol_p + 1e-45, tol_m + 1e-45, tol_v + 1e-45))
    return out


def check_adam(impl, entry, start, wd):
    """entry: 'step' (host step count), 'step_dev' (the count read from device memory), 'multi' (every tensor in one launch, grad_scale 0.5,
    zero_grad)."""
    dev = dev_of(impl)
    hp = dict(ADAM_HP, weight_decay=wd)
    states = [adam_state(n, start, seed=n) for n in ADAM_N]
    gs = 0.5 if entry == "multi" else 1.0
    refs = [adam_ref(p, m, v, grads, start, wd, gs) for p, m, v, grads in states]
    wrong = [adam_ref(p, m, v, grads, start, wd, gs, bias_correction=False) for p, m, v, grads in states]
    live = [[t.clone().to(dev) for t in (p, m, v)] + [torch.zeros_like(p).to(dev)] for p, m, v, _ in states]
    # with the betas as exact doubles: beta2 crosses the ABI rounded by at most half an fp32 ulp (2^-25 in [0.5, 1)), which moves
    # v = b2 v + (1 - b2) g^2 by at most 2^-25 (v + g^2) <= 2^-25 / (1 - b2) of the new v per step (3e-5 for 0.999; 1.3e-5 in fact)
    exact = [adam_ref(p, m, v, grads, start, wd, gs, hp=ADAM_HP_EXACT) for p, m, v, grads in states]
    tab = adam_table(impl, [(p, g, m, v) for p, m, v, g in live], dev) if entry == "multi" else None
    for k in range(ADAM_STEPS):
        step = start + k
        for (p, m, v, g), st in zip(live, states):
            g.copy_(st[3][k].to(dev))
        if entry == "multi":
            impl.adam_multi(tab, step, grad_scale=gs, zero_grad=True, **hp)
        else:
            for p, m, v, g in live:
                impl.adam_step(p, g, m, v, torch.tensor([step], dtype=torch.int32, device=dev) if entry == "step_dev" else step, **hp)
        for n, (p, m, v, g), rf, wr, ex in zip(ADAM_N, live, refs, wrong, exact):
            tag = f"adam_{entry}[n={n} step={step} wd={wd}]"
            rp, rm, rv, tol_p, tol_m, tol_v = rf[k]
            _cmp(tag + ".param", p, rp, tol_p)
            _cmp(tag + ".exp_avg", m, rm, tol_m)
            _cmp(tag + ".exp_avg_sq", v, rv, tol_v)
            _cmp(tag + ".exp_avg_sq vs exact betas", v, ex[k][2], tol_v + (k + 1) * 2.0 ** -25 / (1 - ADAM_HP_EXACT["beta2"]) * ex[k][2])
            if entry == "multi":
                assert bool((g == 0).all()), tag + ": zero_grad left gradients behind"
            if start == 1 and n >= 255:          # at step 10 000 the bias corrections have vanished: nothing to tell apart
                far(tag + ".param vs no bias correction", p, wr[k][0], tol_p)


def check_adam_skip(impl):
    """A set skip flag: parameters and moments bit-unchanged, gradients cleared."""
    dev = dev_of(impl)
    states = [adam_state(n, 10000, seed=n) for n in ADAM_N]
    live = [[t.clone().to(dev) for t in (p, m, v, grads[0])] for p, m, v, grads in states]
    quads = [(p, g, m, v) for p, m, v, g in live]
    tab = adam_table(impl, quads, dev)
    impl.adam_multi(tab, 10000, zero_grad=True, skip=torch.tensor([3], dtype=torch.int32, device=dev), weight_decay=0.01, **ADAM_HP)
    for n, (p, m, v, g), (p0, m0, v0, _) in zip(ADAM_N, live, states):
        assert bits_equal(p, p0) and bits_equal(m, m0) and bits_equal(v, v0), f"adam_multi skip[n={n}]: state changed"
        assert bool((g == 0).all()), f"adam_multi skip[n={n}]: gradients not cleared"


# ---------------------------------------------------------------------------------------------------------------------------------
# argmax of log_softmax: one wave per row, lane l owns classes l, l + 64, ...; ties go to the first index
# ---------------------------------------------------------------------------------------------------------------------------------
ARGMAX_C = (1, 63, 64, 65, 1000, 4096)
ARGMAX_N = (1, 3, 5)
ARGMAX_GAP = 1e-3


def argmax_inputs(n, c, scale):
    """Rows 0 mod 3: a clear winner (gap 1e-2 of the scale) | 1 mod 3: all equal | 2 mod 3: an exact tie of the two largest entries, the
    first of them owned by a HIGHER lane than the second where C allows it (classes 70 and 129: lanes 6 and 1; C = 65: classes 5 and 64:
    lanes 5 and 0; below that every class has a lane of its own: classes 5 and 40).  -> (buffer (n, c + 3), expected first index, last index of the maximum)."""
    g = gen(1000 * n + c + int(scale))
    lb = torch.randn(n, c + 3, generator=g) * scale
    x = lb[:, :c]
    for r in range(n):
        top = int(x[r].argmax())
        x[r, top] += 1e-2 * scale * max(1.0, float(x[r].abs().max()) / scale)
        if r % 3 == 1:
            x[r] = 0.37 * scale
        elif r % 3 == 2 and c >= 63:
            i, j = (70, 129) if c >= 130 else (5, 64) if c == 65 else (5, 40)
            x[r, i] = x[r, j] = x[r, top] + scale
    xd = x.double()
    mx = xd.amax(1, keepdim=True)
    first = (xd == mx).float().argmax(1)
    last = c - 1 - (xd == mx).flip(1).float().argmax(1)
    return lb, first, last


def argmax_gap_ok(x):
    """The input condition: the float64 top-2 gap of every row is exactly 0 or above ARGMAX_GAP x the row's scale (its largest magnitude)."""
    xd = x.double()
    if xd.shape[1] == 1:
        return True
    top2 = xd.topk(2, dim=1).values
    gap = top2[:, 0] - top2[:, 1]
    return bool(((gap == 0) | (gap > ARGMAX_GAP * xd.abs().amax(1))).all())


def check_argmax(impl, c):
    dev = dev_of(impl)
    for n in ARGMAX_N:
        for scale in (1.0, 1e4):
            lb, first, last = argmax_inputs(n, c, scale)
            assert argmax_gap_ok(lb[:, :c])
            ib = torch.full((n + 2,), -7, dtype=torch.int64, device=dev)
            impl.argmax_logsoftmax(lb.to(dev)[:, :c], ib[1:n + 1])
            tag = f"argmax_logsoftmax[{n}x{c} scale={scale}]"
            assert int(ib[0]) == -7 and int(ib[-1]) == -7, tag + ": wrote outside the index block"
            got = ib[1:n + 1].cpu()
            print(f"{tag}: {int((got != first).sum())} of {n} rows differ")
            assert torch.equal(got, first), (tag, got.tolist(), first.tolist())
            if n >= 3 and c >= 63:
                assert not torch.equal(got, last), tag + ": the data cannot tell the first maximum from the last"


# ---------------------------------------------------------------------------------------------------------------------------------
# rotations (rot_math.h): axis-angle <-> 6-D, merge_parts
# ---------------------------------------------------------------------------------------------------------------------------------
ROT_ANGLES = (0.0, 1e-8, 9e-7, 1.1e-6, 1e-3, math.pi / 2, math.pi - 1e-3, math.pi, math.pi + 1e-3, 2 * math.pi - 1e-3, 3 * math.pi)
ROT_ANGLE_NAMES = ("0", "1e-8", "9e-7", "1.1e-6", "1e-3", "pi/2", "pi-1e-3", "pi", "pi+1e-3", "2pi-1e-3", "3pi")
ROT_VARIANTS = ("plain", "x1e-3", "x1e3", "a2 += 0.7 a1")
ROT_DEGENERATE = ("a1 = 0", "a2 || a1", "all zero")
ROT_FLOOR = 8 * EPS32


@functools.lru_cache(maxsize=None)
def rot_axes():
    e = torch.eye(3, dtype=torch.float64)
    r = torch.randn(10, 3, generator=gen(55), dtype=torch.float64)
    return torch.cat([e, -e, r / r.norm(dim=1, keepdim=True)])                       # 16 axes


@functools.lru_cache(maxsize=None)
def rot_aa():
    """(11 angles, 16 axes, 3) float64 -> fp32: the kernels' input; cls[i] = angle index."""
    ang = torch.tensor(ROT_ANGLES, dtype=torch.float64).view(-1, 1, 1)
    return (ang * rot_axes().view(1, 16, 3)).float()


def aa_to_matrix64(aa):
    return orc.quaternion_to_matrix(orc.axis_angle_to_quaternion(aa.double()))


def check_aa_to_rot6d(impl):
    """Well conditioned: each entry is a polynomial of cos / sin of half the angle, whose fp32 argument carries EPS32 x angle.
    tol = 8 EPS32 (1 + angle) per entry (entries are at most 1)."""
    dev = dev_of(impl)
    aa = rot_aa()
    got = impl.axis_angle_to_rot6d(aa.to(dev)).cpu()                                  # the op allocates its output: no canary to check
    ref = orc.axis_angle_to_rotation_6d(aa.double())
    tol = (8 * EPS32 * (1 + torch.tensor(ROT_ANGLES, dtype=torch.float64))).view(11, 1, 1).expand(11, 16, 6)
    errs = []
    for i, nm in enumerate(ROT_ANGLE_NAMES):
        errs.append(_cmp(f"axis_angle_to_rot6d[angle {nm}]", got[i], ref[i], tol[i]))
    assert torch.equal(got[0], torch.tensor([1.0, 0, 0, 0, 1, 0]).expand(16, 6)), "angle 0 is the identity, exactly"
    # wrong reference: the small-angle branch missing, evaluated in fp32 as the kernel would.  0.5 - angle^2 / 48 is the Taylor series of
    # sin(angle / 2) / angle, so for every non-zero angle of the table (also either side of the 1e-6 threshold) the two forms agree to fp32
    # rounding and no threshold could be told from another; what the branch is for is angle 0, where the quotient is 0 / 0 = NaN
    ang = aa.norm(dim=-1, keepdim=True)
    q = torch.cat([torch.cos(ang / 2), aa * (torch.sin(ang / 2) / ang)], -1)
    wrong = orc.quaternion_to_matrix(q)[..., :2, :].reshape(11, 16, 6)
    assert bool(torch.isnan(wrong[0]).all()) and bool(torch.isfinite(wrong[1:]).all())
    _cmp("axis_angle_to_rot6d: the branch-free fp32 form at the non-zero angles", wrong[1:], ref[1:], tol[1:])
    far("axis_angle_to_rot6d vs no small-angle branch", got, wrong, tol)
    return errs


@functools.lru_cache(maxsize=None)
def rot6d_inputs():
    """-> (regular (4 variants, 11, 16, 6) fp32, degenerate (3, 11, 16, 6) fp32), built in float64 from the rotations of `rot_aa`."""
    d6 = orc.axis_angle_to_rotation_6d((torch.tensor(ROT_ANGLES, dtype=torch.float64).view(-1, 1, 1) * rot_axes().view(1, 16, 3)))
    a1, a2 = d6[..., :3], d6[..., 3:]
    reg = torch.stack([d6, d6 * 1e-3, d6 * 1e3, torch.cat([a1, a2 + 0.7 * a1], -1)])
    deg = torch.stack([torch.cat([torch.zeros_like(a1), a2], -1), torch.cat([a1, 2.0 * a1], -1), torch.zeros_like(d6)])
    return reg.float(), deg.float()


@functools.lru_cache(maxsize=None)
def rot6d_refs():
    """float64 rotation matrices of the regular inputs; of the degenerate ones (whose Gram-Schmidt frame is no rotation) the matrix of the
    float64 run of the reference algorithm; and the per-class error of the FP32 oracle functions on the CPU against them:
    class = angle for the regular inputs (pooled over the four variants), one class per degenerate kind."""
    reg, deg = rot6d_inputs()
    r_reg = orc.rotation_6d_to_matrix(reg.double())
    r_deg = aa_to_matrix64(orc.rotation_6d_to_axis_angle(deg.double()))
    o_reg, o_deg = orc.rotation_6d_to_axis_angle(reg), orc.rotation_6d_to_axis_angle(deg)
    e_reg = (aa_to_matrix64(o_reg) - r_reg).abs().amax((-1, -2))                     # (4, 11, 16)
    e_deg = (aa_to_matrix64(o_deg) - r_deg).abs().amax((-1, -2))                     # (3, 11, 16); NaN where either run is not finite
    cls_reg = torch.nan_to_num(e_reg, nan=math.inf).amax((0, 2))                     # (11,)
    cls_deg = torch.nan_to_num(e_deg, nan=math.inf).amax((1, 2))                     # (3,)
    return r_reg, r_deg, o_reg, o_deg, cls_reg, cls_deg


def rot_tol(cls_err):
    """The kernel reproduces the oracle's operation order up to 1-ulp sinf / atan2f differences, which the ill-conditioning of
    sqrt(1 + trace) near angle 0 and pi amplifies as it amplifies the oracle's own error: 4 x the class maximum of the fp32 oracle's
    error, floor 8 EPS32."""
    return torch.clamp(4 * cls_err, min=ROT_FLOOR)


def check_rot6d_to_aa(impl):
    """In matrix space: R(aa_kernel), rebuilt in float64, against the float64 R.  -> the table rows (class, oracle error, kernel error)."""
    dev = dev_of(impl)
    reg, deg = rot6d_inputs()
    r_reg, r_deg, o_reg, o_deg, cls_reg, cls_deg = rot6d_refs()
    allin = torch.cat([reg.reshape(-1, 6), deg.reshape(-1, 6)])
    got = impl.rot6d_to_axis_angle(allin.to(dev)).cpu()
    g_reg, g_deg = got[:reg.numel() // 6].view(4, 11, 16, 3), got[reg.numel() // 6:].view(3, 11, 16, 3)
    assert bool(torch.isfinite(g_reg).all())
    table = []
    err = (aa_to_matrix64(g_reg) - r_reg).abs().amax((-1, -2))
    tol = rot_tol(cls_reg)
    for i, nm in enumerate(ROT_ANGLE_NAMES):
        e = float(err[:, i].max())
        table.append((f"angle {nm}", float(cls_reg[i]), e))
        print(f"rot6d_to_axis_angle[angle {nm}]: fp32 oracle err {float(cls_reg[i]):.3e}, kernel err {e:.3e} (tol {float(tol[i]):.3e})")
        assert e <= float(tol[i]), (nm, e, float(tol[i]))
    # degenerate inputs: finite wherever the fp32 oracle is, and inside the same rule against the float64 run of the algorithm
    fin = torch.isfinite(o_deg).all(-1)
    assert bool(torch.isfinite(g_deg[fin]).all()), "not finite where the fp32 oracle is"
    err_d = (aa_to_matrix64(g_deg) - r_deg).abs().amax((-1, -2))
    tol_d = rot_tol(cls_deg)
    for i, nm in enumerate(ROT_DEGENERATE):
        sel = fin[i] & torch.isfinite(r_deg[i]).all(-1).all(-1)
        e = float(err_d[i][sel].max()) if bool(sel.any()) else 0.0
        table.append((nm, float(cls_deg[i]), e))
        print(f"rot6d_to_axis_angle[{nm}]: fp32 oracle err {float(cls_deg[i]):.3e}, kernel err {e:.3e} (tol {float(tol_d[i]):.3e}), {int(sel.sum())} of 176 finite")
        assert e <= float(tol_d[i]), (nm, e, float(tol_d[i]))
    # wrong reference: the signs of the quaternion's vector part dropped (every axis reflected into the positive octant)
    wrong = aa_to_matrix64(orc.rotation_6d_to_axis_angle(reg.double()).abs())
    i = ROT_ANGLE_NAMES.index("pi/2")
    assert float((aa_to_matrix64(g_reg)[:, i] - wrong[:, i]).abs().max()) > FAR * float(tol[i])
    return table


MERGE_WIDTHS = (106, 78, 180, 61)               # face (jaw 6-D + 100 expression), upper 13 joints, hands 30, lower 9 + 7 translation / contact
MERGE_JOINTS = ([orc.JAW_JOINT], orc.UPPER_JOINTS, orc.HANDS_JOINTS, orc.LOWER_JOINTS)


def check_merge_parts(impl, m):
    """Every part present or absent; the structured 6-D inputs above in the joint slots.  aa layout in matrix space and motion layout (the
    first two rows of R(aa)) against float64 under the 4 x rule of the slot's class (+ the aa -> 6-D tolerance); copies exact."""
    dev = dev_of(impl)
    reg, _ = rot6d_inputs()
    r_reg, _, _, _, cls_reg, _ = rot6d_refs()
    pool, pool_r = reg.reshape(-1, 6), r_reg.reshape(-1, 3, 3)
    pool_cls = torch.arange(11).view(1, 11, 1).expand(4, 11, 16).reshape(-1)
    g = gen(400 + m)
    pick = torch.randperm(pool.shape[0], generator=g)[:m * 53].view(m, 53)            # 53 joint slots per frame
    pick[0, 0] = ROT_ANGLE_NAMES.index("pi/2") * 16 + 7                               # frame 0's jaw: a quarter turn, far from the identity
    parts, slot0 = [], 0
    for w, joints in zip(MERGE_WIDTHS, MERGE_JOINTS):
        p = torch.randn(m, w + 3, generator=g)
        p[:, :6 * len(joints)] = pool[pick[:, slot0:slot0 + len(joints)]].reshape(m, -1)
        parts.append(p)
        slot0 += len(joints)
    ident = torch.eye(3, dtype=torch.float64)
    for present in range(16):
        use = [bool(present >> i & 1) for i in range(4)]
        tag = f"merge_parts[M={m} parts={''.join('FUHL'[i] if use[i] else '-' for i in range(4))}]"
        args = [p.to(dev)[:, :w] if u else None for p, w, u in zip(parts, MERGE_WIDTHS, use)]
        aa, motion, expr = impl.merge_parts(*args, m, dev)
        aa, motion, expr = aa.cpu(), motion.cpu(), expr.cpu()
        ref_r = ident.expand(m, 55, 3, 3).clone()
        tol = torch.full((m, 55), ROT_FLOOR, dtype=torch.float64)
        wrong_r = ref_r.clone()
        slot0 = 0
        for joints, u in zip(MERGE_JOINTS, use):
            if u:
                sel = pick[:, slot0:slot0 + len(joints)]
                ref_r[:, joints] = pool_r[sel]
                tol[:, joints] = rot_tol(cls_reg)[pool_cls[sel]]
                wrong_r[:, [j + 1 if j == orc.JAW_JOINT else j for j in joints]] = pool_r[sel]       # the jaw one joint too far
            slot0 += len(joints)
        got_r = aa_to_matrix64(aa.view(m, 55, 3))
        err = (got_r - ref_r).abs().amax((-1, -2))
        print(f"{tag}.aa: max err {float(err.max()):.3e}, worst err / tol {float((err / tol).max()):.2f}")
        assert bool((err <= tol).all()), tag + ".aa"
        tol6 = tol + 8 * EPS32 * (1 + aa.view(m, 55, 3).double().norm(dim=-1))
        err6 = (motion[:, :330].double().view(m, 55, 6) - ref_r[:, :, :2].reshape(m, 55, 6)).abs().amax(-1)
        print(f"{tag}.motion: max err {float(err6.max()):.3e}, worst err / tol {float((err6 / tol6).max()):.2f}")
        assert bool((err6 <= tol6).all()), tag + ".motion"
        absent = [j for joints, u in zip(MERGE_JOINTS, use) if not u for j in joints] + [23, 24]
        assert bool((aa.view(m, 55, 3)[:, absent] == 0).all()), tag + ": absent joints are zero"
        assert torch.equal(motion[:, :330].view(m, 55, 6)[:, absent], torch.tensor([1.0, 0, 0, 0, 1, 0]).expand(m, len(absent), 6)), tag
        assert torch.equal(motion[:, 330:], parts[3][:, 54:61] if use[3] else torch.zeros(m, 7)), tag + ": translation / contact columns are copies"
        assert torch.equal(expr, parts[0][:, 6:106] if use[0] else torch.zeros(m, 100)), tag + ": expression columns are copies"
        if use[0]:
            assert float((got_r[0, 22:24] - wrong_r[0, 22:24]).abs().max()) > FAR * float(tol[0, 22]), tag + ": the data cannot place the jaw"


# ---------------------------------------------------------------------------------------------------------------------------------
# velocity_to_position (motion.hip): LDS-staged scan up to T = 5120, the one-thread-per-(clip, axis) kernel above
# ---------------------------------------------------------------------------------------------------------------------------------
VEL_CASES = [(2, t, col0, init) for t in (1, 2, 5120, 5121) for col0 in (0, 54) for init in ("per_clip", "shared", "strided")] \
    + [(23, 5121, col0, init) for col0, init in ((0, "per_clip"), (54, "shared"), (54, "strided"))]      # 69 threads: two blocks of 64
VEL_DT = f32(1 / 30)


@functools.lru_cache(maxsize=None)
def vel_inputs(b, t, col0):
    g = gen(1000 * b + t + col0)
    return torch.randn(b * t, col0 + 3 + (4 if col0 else 2), generator=g), torch.randn(b, 5, 3, generator=g)


@functools.lru_cache(maxsize=None)
def vel_refs(b, t, col0, init_kind):
    """-> (float64 recurrence, the same with pos[t] taking v[t] (off by one), sequential fp32 recurrence), each (b, t, 3)."""
    vel, ib = vel_inputs(b, t, col0)
    init = ib[:1, 0].expand(b, 3) if init_kind == "shared" else ib[:, 0]
    v = vel[:, col0:col0 + 3].reshape(b, t, 3)

    def scan(v, init, shift=0):
        pos = torch.cumsum(torch.cat([torch.zeros_like(v[:, :1]), v[:, shift:t - 1 + shift] * VEL_DT], 1), 1) + init.unsqueeze(1)
        pos[:, :, 1] = v[:, :, 1]
        return pos

    seq = [init.clone()]
    for i in range(1, t):
        seq.append(v[:, i - 1] * VEL_DT + seq[-1])
    seq = torch.stack(seq, 1)
    seq[:, :, 1] = v[:, :, 1]
    wrong = scan(v.double(), init.double(), 1) if t > 1 else scan(v.double(), torch.zeros_like(init).double())
    return scan(v.double(), init.double()), wrong, seq


def check_velocity(impl, b, t, col0, init_kind):
    dev = dev_of(impl)
    vel, ib = vel_inputs(b, t, col0)
    ibd = ib.to(dev)
    init = {"per_clip": ibd[:, 0].contiguous(), "shared": ibd[:1, 0].contiguous(), "strided": ibd[:, 0]}[init_kind]
    got = impl.velocity_to_position(vel.to(dev), col0, init, VEL_DT, b, t).cpu()
    ref, wrong, seq = vel_refs(b, t, col0, init_kind)
    tag = f"velocity_to_position[B={b} T={t} col0={col0} init={init_kind}]"
    assert torch.equal(got, seq), f"{tag}: not the sequential fp32 recurrence, max err {float((got - seq).abs().max()):.3e}"
    tol = max(t, 1) * EPS32 * float(ref[:, :, (0, 2)].abs().max())                     # T steps, each rounding at the magnitude of pos
    _cmp(tag, got, ref, tol)
    far(tag + (" vs pos[t] taking v[t]" if t > 1 else " vs zero start"), got, wrong, tol)
