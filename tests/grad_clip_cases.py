"""The case table of the gradient-norm / clipping kernels (csrc/optim.hip: emage_grad_sumsq_multi, emage_adam_multi_scaled,
emage_scale_multi): seeded inputs, float64 references, tolerances derived from the arithmetic.

Every `check_*` takes `impl`: `pantomatrix_amd.ops` (the HIP kernels on the device: tests/test_grad_clip_gpu.py) or `tests/fake_ops.py` with
the stand-ins of tests/fake_grad_clip.py attached (torch on the CPU: tests/test_grad_clip_host.py).

Sums of squares.  The reference is the EXACT float64 dot product: every fp32 value squared in float64 (exact: 48 significant bits) and the
squares added by math.fsum (the correctly rounded sum).  A float64 sum of n non-negative terms in ANY order is within (n - 1) 2^-53 relative
of the exact sum, so the kernel must be within n 2^-53 of this reference, whatever its order.  norm and coef are one fp32 rounding of the
float64 formula (plus the sum's error, far below an fp32 ulp): within 1 fp32 ulp."""
import functools
import math

import numpy as np
import torch

import forward_cases as fc
from pantomatrix_amd import ops

CHUNK = 4096                          # emage_adam_multi_chunk(): elements per block
EDGE_N = (1, 3, 255, 256, 257, 4095, 4096, 4097, 3 * 4096 + 5)       # one thread | a partial wave | around the block width | around a chunk | 4 blocks
N_SMALL = 500                         # more tensors than the model's 481, of 1..7 elements: the finalize pass loops over its waves
N_LARGE = 1_200_003                   # 293 blocks: more partials than the 64 lanes of the wave that adds them
U64 = 2.0 ** -53
NORM_CASES = ((1.0, 0.99), (0.5, 1e31), (1.0 / 3.0, 3.0e38), (1.0, 0.0), (1.0, math.inf), (0.5, None))      # (pre_scale, max_norm)


def sizes():
    g = fc.gen(7)
    small = torch.randint(1, 8, (N_SMALL,), generator=g).tolist()
    return list(EDGE_N) + small + [N_LARGE]


def values(n, seed):
    """Mixed signs, magnitudes 10^U(-30, 30): an fp32 square would flush the small ones to zero and overflow on the large ones."""
    g = fc.gen(seed)
    mag = 10.0 ** (60.0 * torch.rand(n, generator=g, dtype=torch.float64) - 30.0)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    return (mag * sign).to(torch.float32)


def off16_view(x, dev):
    """A copy of x on `dev` as a view that starts ONE FLOAT past a 16-byte boundary (gradient bucket views are 4-byte aligned only)."""
    buf = torch.zeros(x.numel() + 8, dtype=torch.float32, device=dev)
    skip = (4 - (buf.data_ptr() % 16) // 4) % 4 + 1
    v = buf[skip:skip + x.numel()]
    assert v.data_ptr() % 16 == 4
    v.copy_(x)
    return v


class HostTable:
    """What the CPU stand-ins read of an `ops.AdamTable`."""

    def __init__(self, quads, device):
        self.keep = quads


def table(impl, grads, dev):
    """A table over gradients only (the parameter / moment words are not read by the norm and scaling kernels)."""
    return (ops.AdamTable if impl is ops else HostTable)([(g, g, g, g) for g in grads], dev)


@functools.lru_cache(maxsize=None)
def big_table():
    """The host tensors of the main case and their exact sums of squares (computed once, shared by the tests, never modified)."""
    xs = [values(n, 1000 + i) for i, n in enumerate(sizes())]
    sq = [math.fsum((x.double() ** 2).tolist()) for x in xs]
    return xs, sq, math.fsum(sq)


def ulp32(x):
    """Spacing of the fp32 numbers at |x| (the smallest subnormal below the normal range)."""
    x = abs(float(x))
    if not math.isfinite(x):
        return math.inf
    return float(np.spacing(np.float32(min(x, 3.4028234e38))))


def formula(total, pre_scale, max_norm):
    """(norm, coef) of include/emage_hip.h in float64."""
    with np.errstate(all="ignore"):
        nrm = np.float64(pre_scale) * np.sqrt(np.float64(total))
        cf = np.float64(1.0)
        mx = 0.0 if max_norm is None else float(max_norm)
        if mx > 0 and not math.isinf(mx):
            cf = np.float64(mx) / (nrm + 1e-6)
            if cf > 1.0:
                cf = np.float64(1.0)
    return float(nrm), float(cf)


def _new_out(impl, tab):
    import fake_grad_clip
    return ops.GradNorm(tab) if impl is ops else fake_grad_clip.new_buffers(tab)


def check_sums(tag, out, counts, sq, total):
    got = out.tensor_sumsq.detach().cpu().tolist()
    worst = 0.0
    for i, (n, want, have) in enumerate(zip(counts, sq, got)):
        rel = abs(have - want) / want if want else abs(have)
        worst = max(worst, rel / (n * U64))
        assert rel <= n * U64, (tag, i, n, have, want, rel)
    n_all = sum(counts)
    have = float(out.total_sumsq)
    rel = abs(have - total) / total if total else abs(have)
    print(f"{tag}: {len(counts)} tensors, worst per-tensor error {worst:.3f} x n 2^-53; total {have:.17e}: {rel / (n_all * U64):.2e} x N 2^-53 (N = {n_all})")
    assert rel <= n_all * U64, (tag, have, total, rel)


def check_scalars(tag, out, total, pre_scale, max_norm):
    nrm, cf = formula(total, pre_scale, max_norm)
    got_n, got_c = float(out.norm), float(out.coef)
    print(f"{tag}: norm {got_n:.9e} (float64 {nrm:.17e}), coef {got_c:.9e} (float64 {cf:.17e})")
    assert abs(got_n - nrm) <= ulp32(nrm), (tag, got_n, nrm)
    assert abs(got_c - cf) <= ulp32(cf), (tag, got_c, cf)
    if max_norm is None or max_norm <= 0 or math.isinf(max_norm):
        assert got_c == 1.0, (tag, got_c)


def out_bits(out):
    return [t.detach().cpu().clone() for t in (out.tensor_sumsq, out.total_sumsq, out.norm, out.coef)]


def check_big_table(impl, pre_scale, max_norm):
    """The main case: edge sizes, 500 tiny tensors and one of 293 blocks in ONE table, every view one float past a 16-byte boundary;
    a second launch into other buffers gives the same bits; the gradients are not modified."""
    dev = fc.dev_of(impl)
    xs, sq, total = big_table()
    grads = [off16_view(x, dev) for x in xs]
    tab = table(impl, grads, dev)
    tag = f"grad_norm[pre_scale={pre_scale:g} max_norm={max_norm}]"
    out = impl.grad_norm(tab, pre_scale, max_norm)
    check_sums(tag, out, [x.numel() for x in xs], sq, total)
    check_scalars(tag, out, total, pre_scale, max_norm)
    first = out_bits(out)
    again = impl.grad_norm(tab, pre_scale, max_norm, out=_new_out(impl, tab))
    assert again is not out
    for a, b in zip(first, out_bits(again)):
        assert fc.bits_equal(a, b), tag + ": two launches differ"
    for x, g in zip(xs, grads):
        assert fc.bits_equal(x, g), tag + ": the gradients were modified"


def check_zero_table(impl):
    """All-zero gradients: norm 0 and coef EXACTLY 1 (max_norm / 1e-6 clamps to 1)."""
    dev = fc.dev_of(impl)
    grads = [off16_view(torch.zeros(n), dev) for n in (1, 257, 4097)]
    out = impl.grad_norm(table(impl, grads, dev), 1.0, 0.99)
    assert float(out.total_sumsq) == 0.0 and float(out.norm) == 0.0 and float(out.coef) == 1.0
    assert out.tensor_sumsq.detach().cpu().tolist() == [0.0, 0.0, 0.0]


def check_one_tensor(impl, n):
    dev = fc.dev_of(impl)
    x = values(n, 50 + n)
    sq = math.fsum((x.double() ** 2).tolist())
    out = impl.grad_norm(table(impl, [off16_view(x, dev)], dev), 1.0, 0.99)
    check_sums(f"grad_norm[one tensor n={n}]", out, [n], [sq], sq)
    check_scalars(f"grad_norm[one tensor n={n}]", out, sq, 1.0, 0.99)


def check_nonfinite(impl, bad):
    """One NaN / one inf element (in the last block of a three-block tensor): the norm is NaN / inf as torch's is, the other tensors' sums
    are untouched, and coef is what the formula gives (NaN stays NaN; max_norm / inf = 0)."""
    dev = fc.dev_of(impl)
    xs = [torch.randn(n, generator=fc.gen(n)) for n in (5, 2 * CHUNK + 77, 300)]
    xs[1][2 * CHUNK + 3] = bad
    out = impl.grad_norm(table(impl, [off16_view(x, dev) for x in xs], dev), 1.0, 0.99)
    per = out.tensor_sumsq.detach().cpu().tolist()
    nrm, cf = float(out.norm), float(out.coef)
    print(f"grad_norm[{bad}]: norm {nrm}, coef {cf}")
    for i in (0, 2):
        want = math.fsum((xs[i].double() ** 2).tolist())
        assert abs(per[i] - want) <= xs[i].numel() * U64 * want
    if math.isnan(bad):
        assert math.isnan(per[1]) and math.isnan(float(out.total_sumsq)) and math.isnan(nrm) and math.isnan(cf)
    else:
        assert per[1] == math.inf and float(out.total_sumsq) == math.inf and nrm == math.inf and cf == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# emage_adam_multi_scaled: the block forms s = grad_scale * coef ONCE in fp32 and runs emage_adam_multi's arithmetic with it, so the
# results are BIT-equal to emage_adam_multi with grad_scale = fp32(fp32(grad_scale) * coef)
# ---------------------------------------------------------------------------------------------------------------------------------
ADAM_N = (1, 4095, 4097)
COEFS = (1.0, 0.5, 0.00201)
GRAD_SCALES = (1.0, 0.125, 1.0 / 3.0)
ADAM_STATES = ((1, 0.0), (1, 0.01), (10002, 0.0), (10002, 0.01))      # (step, weight decay): fresh moments | late, bias corrections ~1


def scaled_adam(impl):
    """`adam_multi` taking `grad_scale_dev` (tests/fake_ops.py's own stand-in predates the keyword: tests/fake_grad_clip.py adds a sibling)."""
    return impl.adam_multi if impl is ops else impl.adam_multi_scaled


def _adam_live(start, dev):
    states = [fc.adam_state(n, start, seed=n) for n in ADAM_N]
    live = [[off16_view(t, dev) for t in (p, m, v, grads[0])] for p, m, v, grads in states]
    return states, live


def check_adam_scaled(impl, coef, grad_scale, start, wd):
    dev = fc.dev_of(impl)
    tag = f"adam_multi_scaled[coef={coef:g} grad_scale={grad_scale:g} step={start} wd={wd}]"
    _, a = _adam_live(start, dev)
    _, b = _adam_live(start, dev)
    tab_a = (ops.AdamTable if impl is ops else HostTable)([(p, g, m, v) for p, m, v, g in a], dev)
    tab_b = (ops.AdamTable if impl is ops else HostTable)([(p, g, m, v) for p, m, v, g in b], dev)
    c = torch.tensor([coef], dtype=torch.float32, device=dev)
    scaled_adam(impl)(tab_a, start, weight_decay=wd, grad_scale=grad_scale, zero_grad=True, grad_scale_dev=c, **fc.ADAM_HP)
    folded = float(np.float32(grad_scale) * np.float32(coef))
    impl.adam_multi(tab_b, start, weight_decay=wd, grad_scale=folded, zero_grad=True, **fc.ADAM_HP)
    for n, ta, tb in zip(ADAM_N, a, b):
        for name, x, y in zip(("param", "exp_avg", "exp_avg_sq", "grad"), ta, tb):
            assert fc.bits_equal(x, y), f"{tag}.{name}[n={n}]"
        assert bool((ta[3] == 0).all()), tag + ": zero_grad left gradients behind"
    states, _ = _adam_live(start, "cpu")
    assert not fc.bits_equal(a[1][0], states[1][0]), tag + ": nothing moved"


def check_adam_scaled_skip(impl):
    """A set skip word: parameters and moments bit-unchanged, gradients cleared — with the device factor as without it."""
    dev = fc.dev_of(impl)
    states, live = _adam_live(10002, dev)
    tab = (ops.AdamTable if impl is ops else HostTable)([(p, g, m, v) for p, m, v, g in live], dev)
    c = torch.tensor([0.5], dtype=torch.float32, device=dev)
    scaled_adam(impl)(tab, 10002, zero_grad=True, skip=torch.tensor([3], dtype=torch.int32, device=dev), weight_decay=0.01, grad_scale_dev=c, **fc.ADAM_HP)
    for n, (p, m, v, g), (p0, m0, v0, _) in zip(ADAM_N, live, states):
        assert fc.bits_equal(p, p0) and fc.bits_equal(m, m0) and fc.bits_equal(v, v0), f"adam_multi_scaled skip[n={n}]: state changed"
        assert bool((g == 0).all()), f"adam_multi_scaled skip[n={n}]: gradients not cleared"


def check_scale_multi(impl):
    """g *= coef over a table: every gradient afterwards is bit-equal to fp32(g * coef)."""
    dev = fc.dev_of(impl)
    xs = [torch.randn(n, generator=fc.gen(3 * n)) for n in (1, 255, 4097, 2 * CHUNK)]
    grads = [off16_view(x, dev) for x in xs]
    c = torch.tensor([0.00201], dtype=torch.float32, device=dev)
    impl.scale_multi(table(impl, grads, dev), c)
    for x, g in zip(xs, grads):
        assert fc.bits_equal(g, x * c.cpu()), f"scale_multi[n={x.numel()}]"
