"""The case tables of the contraction tests: `emage_gemm` (csrc/gemm_tile.h, gemm.hip, h2_tile.h, gemm_h2.hip), the one kernel family behind every
Linear and Conv1d, in F32, BF16, F16X3 and H2, against a float64 reference built from the stored operands with plain indexing (a row gather, one
einsum), with the tolerance derived from the kernel's arithmetic per entry and one plausible WRONG reference per feature.

Every `check_*` takes `impl`: `pantomatrix_amd.ops` (tests/test_gemm_float64_gpu.py) or `tests/fake_ops.py` / torch's own fp32 code behind the `gemm`
signature (tests/test_gemm_float64_host.py).  Conventions as in tests/forward_cases.py and tests/attention_lstm_cases.py: every operand and output
is an offset, strided view of a NaN-filled buffer, every output buffer must still be NaN outside its block, every comparison goes through `_cmp` and
prints its max error, a wrong reference must miss by more than FAR x the tolerance, and what crosses the C ABI as `float` (w_scale) is a power of two.

Inputs of EVERY case: A's channels [C, Cp) hold 1e3 (the contract: "finite, they meet zero weights"), lda = Cp + 64 with the columns past Cp and
the rows before and after A NaN, W a view 64 elements into a NaN buffer, bias / slope views 4 elements into NaN buffers, the residual and the
outputs blocks of NaN buffers with their own pitches.  N(0,1) draws are clamped to +-4 so that the rows scaled 1e3 keep |a| * 16 < 65504.

Tolerance per entry (u = EPS32 = 2^-24; rounding model of tests/attention_lstm_cases.py: an fp32 sum of K terms in any order is within K u S of the
exact one, S = sum |a||w| in float64):
  contraction   F32 / BF16 (exact products of the stored operands, fp32 accumulation):  K u S
                F16X3 / H2:  (SPLIT_REL + 3 K u) S + (SPLIT_FLOOR / a_scale) sum_{a != 0} |w| + (SPLIT_FLOOR / w_scale) sum_{w != 0} |a|
                (the floors are those of the low planes where they are fp16 subnormals; an operand that is exactly 0 splits into 0 + 0 and pays none:
                this is what keeps the zero rows, the pad-only outputs and the 1e3 channel tail against zero weights exact)
  epilogue      + u (|x| + |y|) per addition x + y (bias, residual: the larger of intermediate and result is covered), + u |v s| for the slope; the
                activation has Lipschitz constant max(1, |s|) = 1 for the slopes used, so what came in goes through unchanged; an H2 residual is
                decoded as (hi + lo) / 16 in fp32: + u |res|
  output format bf16 `out` / `out_t`: + 2^-8 relative; H2 image: + 2^-22 relative + SPLIT_FLOOR / 16; fp32: nothing
On top, every F16X3 / H2 case is held to the project's "4 x" rule, per row: the error against float64 may be at most 4 x the largest error in that row
of the F32 restatement of the same case — `fake_ops.gemm` with F32 on the CPU, fed the very A, W, bias, slope and residual values of the case under
test (`f32_restatement_error`) — floor 8 EPS32 S per entry, PLUS the two floor terms above (and the output format's term): the floor terms are
absolute errors of the split that fp32 arithmetic does not have, and at rows scaled 1e-4 (a * 16 ~ 2^-9: the low plane is a subnormal with spacing
2^-24, i.e. 2^-16 of the value) they are the whole error; without them the CPU restatement of the split itself misses the rule there, by a factor
of 16 at the 64 x 64 `kinds` case.  Nothing else is added: the epilogue's roundings are the restatement's too.

A wrong reference is judged only where it is finite (`far_finite`), and what it reads beyond the data of the right one is finite neighbouring
data wherever the layout has any, so that every rejection is made by the values.

H2 `out`: an image row is stored in whole groups of 8 columns (the host pads the row), so the kernel also writes the columns between
max(N, n_store) and the next multiple of 8: they are exactly +0 in both planes, like the zero-filled tail."""
import dataclasses
import functools
import zlib

import torch

import fake_ops as F
from forward_cases import dev_of, far, gen, nans
from kernel_checks import EPS32, SPLIT_FLOOR, SPLIT_REL, _cmp, _nan_outside
from pantomatrix_amd import ops
from pantomatrix_amd._lib import BF16, F32, F16X3, H2

DTYPES = {"f32": F32, "bf16": BF16, "f16x3": F16X3, "h2": H2}
SPLIT = ("f16x3", "h2")
BF16_HALF_ULP = 2.0 ** -8
H2_REL = 2.0 ** -22
TAIL = 1e3                 # A's channels [C, Cp)
LOUD, QUIET = 1e2, 1e-1    # `loud` convolution cases: the neighbouring sequences hold values LOUD / QUIET = 1e3 times those of the sequence under test (the
                           # middle one); split so that the loud outputs (~ 5e2) stay inside the range of an H2 output image (|x| < 4094)
CLAMP = 4.0
KINDS = ("N(0,1)", "1e-4 N(0,1)", "1e3 N(0,1)", "cancelling", "zero")      # kind of input row r of a `kinds` case: r % 5
A_COL0, OUT_COL0, F32_COL0, RES_COL0 = 16, 8, 24, 16                       # column offsets of the blocks inside their buffers (16-byte aligned)


@dataclasses.dataclass(frozen=True)
class Case:
    """One `gemm` call.  Linear: nb = 1 and lin = lout = m.  slope: None, a number or "vec" (first half 0.01, second half 1); res: None, "lo" (the
    storage dtype), "f32" or "h2" (an H2 image, H2 only: `for_dtype` turns it into "lo" elsewhere); outs: "out", "f32", "both", "none" (only out_t);
    t_col0 None = no transposed tail; t_pad: t_ld = round_up(t_rows, 32) + t_pad; rows: the output rows the float64 reference is computed for
    (None = all)."""
    m: int
    n: int
    cp: int
    c: int = 0
    nb: int = 1
    lin: int = 0
    lout: int = 0
    taps: int = 1
    stride: int = 1
    pad: int = 0
    bias: bool = True
    slope: object = None
    res: object = None
    res_first: bool = False
    outs: str = "out"
    n_store: int = 0
    t_col0: object = None
    t_rows: int = 0
    t_pad: int = 0
    kinds: bool = False
    loud: bool = False
    sample: bool = False

    def __post_init__(self):
        for k, v in (("c", self.cp), ("lin", self.m // self.nb), ("lout", self.m // self.nb)):
            if not getattr(self, k):
                object.__setattr__(self, k, v)
        assert self.m == self.nb * self.lout and self.cp % 64 == 0 and 0 < self.c <= self.cp
        assert self.outs != "none" or self.t_col0 == 0

    @property
    def ncol(self):
        return self.n if self.t_col0 is None else self.t_col0

    @property
    def identity(self):
        return self.taps == 1 and self.stride == 1 and self.pad == 0 and self.lin == self.lout

    def tag(self, name):
        geo = "" if self.identity else f" taps={self.taps} stride={self.stride} pad={self.pad} Lin={self.lin} Lout={self.lout} nb={self.nb}"
        ep = f" bias={int(self.bias)} slope={self.slope} res={self.res}{'(first)' if self.res and self.res_first else ''} outs={self.outs}"
        tail = (f" n_store={self.n_store}" if self.n_store else "") + (f" t_col0={self.t_col0} t_rows={self.t_rows} t_pad={self.t_pad}" if self.t_col0 is not None else "")
        return f"gemm[{name} M={self.m} N={self.n} Cp={self.cp} C={self.c}{geo}{ep}{tail}{' kinds' if self.kinds else ''}{' loud' if self.loud else ''}]"

    def for_dtype(self, name):
        return dataclasses.replace(self, res="lo") if self.res == "h2" and name != "h2" else self

    def ident(self):
        return "-".join(str(getattr(self, f.name)) for f in dataclasses.fields(self))


def lin(m, n, cp, **kw):
    return Case(m=m, n=n, cp=cp, **kw)


def conv(geo, nb, cp, n, **kw):
    taps, stride, pad, li, lo = geo
    kw.setdefault("slope", 0.2)
    kw.setdefault("outs", "both")
    return Case(m=nb * lo, n=n, cp=cp, nb=nb, lin=li, lout=lo, taps=taps, stride=stride, pad=pad, n_store=128 if n == 106 else 0, **kw)


# ---------------------------------------------------------------------------------------------------------------------------------
# table 1: the Linear grid (the heuristic takes the 64 x 64 tile at these sizes), the zero-filled tail, the transposed tail
# ---------------------------------------------------------------------------------------------------------------------------------
LINEAR_M, LINEAR_N, LINEAR_CP = (1, 63, 64, 65, 129), (1, 7, 8, 9, 63, 64, 65, 200), (64, 192, 448)
LINEAR_GRID = [
    # every M, N, Cp, C in {Cp, Cp - 27}; bias x slope x res x res_first x outs pairwise; `kinds` at a ragged shape (65 x 63) and a full tile (64 x 64)
    lin(1, 1, 64, bias=True, slope=None, res=None, outs="out"),
    lin(1, 200, 448, c=421, bias=False, slope=0.2, res="f32", res_first=True, outs="both"),
    lin(63, 7, 192, c=165, bias=True, slope=0.0, res="lo", outs="f32"),
    lin(63, 64, 64, c=37, bias=False, slope="vec", res="h2", res_first=True, outs="out"),
    lin(64, 8, 448, bias=True, slope=1.0, res="f32", outs="out"),
    lin(64, 64, 192, c=165, bias=True, slope=0.2, res="lo", res_first=True, outs="both", kinds=True),
    lin(64, 64, 64, bias=False, slope=None, res=None, outs="f32", kinds=True),
    lin(65, 9, 64, c=37, bias=True, slope="vec", res=None, outs="both"),
    lin(65, 63, 192, bias=True, slope=0.2, res="h2", outs="both", kinds=True),
    lin(65, 63, 448, c=421, bias=False, slope=0.0, res="f32", res_first=True, outs="out", kinds=True),
    lin(65, 65, 192, bias=False, slope=1.0, res="lo", outs="f32"),
    lin(129, 65, 64, bias=True, slope=0.0, res="h2", res_first=True, outs="f32"),
    lin(129, 200, 192, c=165, bias=True, slope="vec", res="f32", outs="out"),
    lin(129, 8, 448, c=421, bias=False, slope=0.2, res=None, outs="both"),
    lin(64, 200, 64, bias=True, slope=None, res="lo", res_first=True, outs="both"),
    lin(63, 9, 448, bias=False, slope=None, res="h2", outs="out"),
]
assert {c.m for c in LINEAR_GRID} == set(LINEAR_M) and {c.n for c in LINEAR_GRID} == set(LINEAR_N) and {c.cp for c in LINEAR_GRID} == set(LINEAR_CP)
assert {c.slope for c in LINEAR_GRID} == {None, 0.0, 0.2, 1.0, "vec"} and {c.res for c in LINEAR_GRID} == {None, "lo", "f32", "h2"}
# (N, n_store): the tail [N, n_store) of `out` is exactly 0 and nothing is written beyond it; (40, 136) crosses a 64-column tile boundary
LINEAR_TAIL = [lin(65, n, 192, c=165, slope=0.2, outs="both", n_store=ns) for n, ns in ((106, 128), (40, 136), (64, 64))]
# transposed tail: every t_rows, t_col0 in {0 (out NULL), 64, N (empty tail)}, nb in {1, 3}, t_ld in {round_up(t_rows, 32), + 32}
LINEAR_T = [
    lin(1, 7, 64, outs="none", t_col0=0, t_rows=1),
    lin(3, 73, 192, c=165, outs="both", slope=0.2, t_col0=64, t_rows=1, t_pad=32),
    lin(17, 128, 64, outs="out", t_col0=128, t_rows=17),
    lin(51, 200, 192, outs="f32", slope="vec", t_col0=64, t_rows=17, t_pad=32),
    lin(64, 72, 64, c=37, outs="none", slope=0.2, t_col0=0, t_rows=64, t_pad=32),
    lin(192, 128, 192, outs="both", t_col0=64, t_rows=64),
    lin(65, 129, 448, c=421, outs="out", slope=0.0, t_col0=64, t_rows=65),
    lin(195, 100, 64, outs="both", bias=False, t_col0=64, t_rows=65, t_pad=32),
    lin(195, 64, 64, outs="f32", t_col0=64, t_rows=65, t_pad=32),
]
assert {c.t_rows for c in LINEAR_T} == {1, 17, 64, 65} and {c.m // c.t_rows for c in LINEAR_T} == {1, 3} and {c.t_pad for c in LINEAR_T} == {0, 32}
LINEAR_CASES = LINEAR_GRID + LINEAR_TAIL + LINEAR_T

# ---------------------------------------------------------------------------------------------------------------------------------
# table 2: convolution geometry (taps, stride, pad, Lin, Lout); nb = 3 puts a sequence boundary inside a 64-row tile
# ---------------------------------------------------------------------------------------------------------------------------------
GEOMETRIES = [(3, 1, 1, 1, 1), (3, 1, 1, 2, 2), (3, 1, 1, 37, 37), (15, 1, 7, 5, 5), (15, 1, 7, 20, 20), (15, 6, 0, 75, 11), (4, 2, 1, 10, 5),
              (3, 5, 0, 23, 5), (3, 1, 4, 6, 12), (3, 1, 1, 40, 37)]
PAD_ONLY = (3, 1, 4, 6, 12)            # pad > taps: outputs 0, 1 and 10, 11 of every sequence see only padding
CONV_CASES = []
for i, geo in enumerate(GEOMETRIES):
    CONV_CASES.append(conv(geo, 3, (64, 128)[i % 2], (106, 64)[i % 2], c=(37, 128)[i % 2], loud=i % 2 == 0, res=(None, "lo")[i % 2], res_first=True))
    CONV_CASES.append(conv(geo, 1, (128, 64)[i % 2], (64, 106)[i % 2], c=(101, 64)[i % 2], loud=False, bias=i % 2 == 0))
assert sum(c.loud for c in CONV_CASES) * 4 >= len(CONV_CASES)

# table 3: taps == 1 with a geometry (a 1 x 1 convolution): the row mapping of include/emage_hip.h holds for every taps
TAPS1_GEOMETRIES = [(1, 2, 0, 20, 10), (1, 1, 1, 10, 12), (1, 3, 0, 31, 11), (1, 1, 0, 12, 10)]
TAPS1_CASES = [conv(geo, 3, 64, 64, c=37, loud=i % 2 == 0) for i, geo in enumerate(TAPS1_GEOMETRIES)] + [conv(TAPS1_GEOMETRIES[0], 3, 128, 106, res="lo")]

# ---------------------------------------------------------------------------------------------------------------------------------
# table 5: every product tile configuration, forced through the tools library (emage_set_tuning key 0 / 4), at small shapes, and once at the
# smallest shape where the product library's heuristic selects it on 256 CUs
# ---------------------------------------------------------------------------------------------------------------------------------
PIPE_TILES = {25: (64, 64), 32: (64, 192), 33: (64, 192), 34: (128, 128), 36: (128, 64)}            # csrc/gemm.hip: PIPE_CONFIGS
H2_TILES = {100: (64, 192), 113: (128, 128), 119: (128, 256), 120: (64, 64), 170: (128, 192)}      # csrc/gemm_h2.hip: H2_CONFIGS


def tile_cases(bm, bn):
    """K = 64 is two K-tiles, fewer than any ring has slots."""
    return [lin(1, bn + 8, 64, slope=0.2, outs="both"),
            lin(bm + 1, bn + 8, 64, c=37, slope="vec", res="f32", outs="both"),
            lin(bm + 1, 40, 64, slope=0.2, outs="out", n_store=bn + 8),
            lin(195, bn + 40, 64, outs="both", slope=0.2, t_col0=bn, t_rows=65),
            conv((3, 1, 1, 37, 37), 3, 64, bn + 8, c=37, loud=True),
            conv((1, 2, 0, 20, 10), 3, 64, bn + 8, loud=True)]


# (configuration the heuristic takes in F32 / BF16, case).  F16X3 takes its own table (csrc/gemm.hip: dispatch) at the same shapes
HEURISTIC_PIPE = [(34, lin(4096, 2304, 64, slope=0.2, outs="out", sample=True)),
                  (33, lin(2048, 3072, 64, slope=0.2, outs="out", sample=True)),
                  (32, lin(2048, 768, 128, slope=0.2, res="f32", outs="out", sample=True)),
                  (36, Case(m=8200, n=64, cp=64, nb=1, lin=8200, lout=8200, taps=15, stride=1, pad=7, slope=0.2, outs="out", sample=True))]
HEURISTIC_H2 = [(100, lin(1024, 1152, 64, slope=0.2, outs="out", sample=True)),
                (113, lin(1024, 1024, 64, slope=0.2, outs="out", sample=True)),
                (119, lin(4096, 4096, 64, slope=0.2, outs="out", sample=True)),
                (170, lin(4096, 6144, 64, slope=0.2, outs="out", sample=True))]


def sample_rows(m):
    """Every row of the first and the last 128-row tile and every 16th row between."""
    if m <= 256:
        return torch.arange(m)
    return torch.cat([torch.arange(128), torch.arange(128, m - 128, 16), torch.arange(m - 128, m)])


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs: the STORED values in float64 and the operands as the kernels take them
# ---------------------------------------------------------------------------------------------------------------------------------
def _rn(g, *shape):
    return torch.randn(*shape, generator=g).clamp_(-CLAMP, CLAMP)


@functools.lru_cache(maxsize=8)
def inputs(name, cs):
    """-> dict: a (nb Lin, Cp), w (N, taps, Cp), bias, slope (N) or None, res (M, N) or None: float64 of the stored values (bf16-rounded for bf16;
    for F16X3 / H2 the fp32 values that get packed; an H2 residual: the value its image holds), and `packed`: the CPU operands."""
    g = gen(zlib.crc32(cs.ident().encode()))
    td = torch.bfloat16 if name == "bf16" else torch.float32
    rows = cs.nb * cs.lin
    a = torch.full((rows, cs.cp), TAIL)
    a[:, :cs.c] = _rn(g, rows, cs.c)
    w = torch.zeros(cs.n, cs.taps, cs.cp)
    w[:, :, :cs.c] = _rn(g, cs.n, cs.taps, cs.c) / (cs.c * cs.taps) ** 0.5
    if cs.kinds:
        assert cs.identity
        w[:, 0, :cs.c] -= w[:, 0, :cs.c].mean(1, keepdim=True)          # rows of W sum to ~0: a constant row of A cancels
        kind = torch.arange(rows) % 5
        a[kind == 1, :cs.c] *= 1e-4
        a[kind == 2, :cs.c] *= 1e3
        a[kind == 3, :cs.c] += 1e3
        a[kind == 4, :cs.c] = 0.0
    if cs.loud:
        seq = torch.arange(rows) // cs.lin
        a[seq != cs.nb // 2, :cs.c] *= LOUD
        a[seq == cs.nb // 2, :cs.c] *= QUIET
    a, w = a.to(td), w.to(td)
    bias = _rn(g, cs.n) if cs.bias else None
    slope = None if cs.slope is None else torch.cat([torch.full((cs.n // 2,), 0.01), torch.ones(cs.n - cs.n // 2)]) if cs.slope == "vec" else torch.full((cs.n,), float(cs.slope))
    res, res_p = None, None
    n8 = ops.round_up(cs.n, 8)
    if cs.res is not None:
        r = _rn(g, cs.m, n8)
        if cs.res == "h2":
            res_p = ops.h2_pack(r)
            hi, lo = F.h2_planes(res_p, n8)
            res = ((hi.double() + lo.double()) / ops.A_SCALE_F16X3)[:, :cs.n]
        else:
            res_p = (r.to(td) if cs.res == "lo" else r)[:, :cs.n]
            res = res_p.double()
    w2 = w.reshape(cs.n, cs.taps * cs.cp)
    ws = 1.0
    if name == "f16x3":
        w_p, ws = ops.split_f16_weights(w2)
    elif name == "h2":
        w_p, ws = ops.split_f16_weights_h2(w2)
    else:
        w_p = w2
    a_p = ops.h2_pack(a) if name == "h2" else a
    dbl = lambda t: None if t is None else t.double()
    return dict(a=a.double(), w=w.double(), bias=dbl(bias), slope=dbl(slope), res=res, ws=ws,
                packed=dict(a=a_p, w=w_p, bias=bias, slope=slope, res=res_p))


# ---------------------------------------------------------------------------------------------------------------------------------
# the float64 reference: row(m, tap) = b Lin + l stride + tap - pad, zero rows outside [0, Lin); then bias, residual, leaky
# ---------------------------------------------------------------------------------------------------------------------------------
def gather(a, cs, rows, *, edge="zero", stride=None, pad=None, reverse=False, pitch=None):
    """-> x (len(rows), taps, Cp): the A rows output row m contracts.  Wrong variants: edge = "neighbour" (no zero padding: the row in front of /
    behind the sequence; in front of / behind A the rows of its other end, finite data like every other neighbour), another stride / pad, the taps
    in reverse order, the batch pitch `pitch` for Lout."""
    stride, pad, pitch = cs.stride if stride is None else stride, cs.pad if pad is None else pad, cs.lout if pitch is None else pitch
    b, l = rows // pitch, rows % pitch
    taps = torch.arange(cs.taps)
    pos = l[:, None] * stride + (taps.flip(0) if reverse else taps)[None, :] - pad
    r = b[:, None] * cs.lin + pos
    inside = (pos >= 0) & (pos < cs.lin)
    if edge == "neighbour":
        return a[r % a.shape[0]]
    return a[r.clamp(0, a.shape[0] - 1)] * inside[:, :, None]


def epilogue(v, cs, inp, rows, *, bias_shift=0, slope_side="neg", res_side=None, res=None):
    """-> (value, u-weighted magnitude sum of the epilogue's roundings).  Wrong variants: the bias of column n + 1, the slope on the positive side,
    the residual on the other side of the activation, another residual."""
    mag = torch.zeros_like(v)
    if inp["bias"] is not None:
        b = inp["bias"].roll(-bias_shift)
        mag += v.abs() + b.abs()
        v = v + b
    r = inp["res"][rows] if res is None and inp["res"] is not None else res
    first = cs.res_first if res_side is None else res_side
    if r is not None and first:
        mag += v.abs() + r.abs()
        v = v + r
    if inp["slope"] is not None:
        v = torch.where((v > 0) if slope_side == "neg" else (v < 0), v, v * inp["slope"])
        mag += v.abs()
    if r is not None and not first:
        mag += v.abs() + r.abs()
        v = v + r
    if r is not None and cs.res == "h2":
        mag += r.abs()
    return v, mag


def reference(name, cs, rows, inp=None):
    """-> dict(ref, tol (before the output format), s, floors, x, w2) for the output rows `rows`, all (len(rows), N) float64.  inp: the stored values
    (default: those of `inputs(name, cs)`)."""
    inp = inputs(name, cs) if inp is None else inp
    x = gather(inp["a"], cs, rows).reshape(len(rows), -1)
    w2 = inp["w"].reshape(cs.n, -1)
    k = cs.taps * cs.cp
    v = x @ w2.t()
    s = x.abs() @ w2.abs().t()
    if name in SPLIT:
        floors = SPLIT_FLOOR / ops.A_SCALE_F16X3 * ((x != 0).double() @ w2.abs().t()) + SPLIT_FLOOR / inp["ws"] * (x.abs() @ (w2 != 0).double().t())
        tol = (SPLIT_REL + 3 * k * EPS32) * s + floors
    else:
        floors = torch.zeros_like(s)
        tol = k * EPS32 * s
    ref, mag = epilogue(v, cs, inp, rows)
    return dict(ref=ref, tol=tol + EPS32 * mag, s=s, floors=floors, mag=mag, x=x, w2=w2, v=v)


def format_tol(name, key, ref, tol):
    if name == "bf16" and key in ("out", "out_t"):
        return tol + BF16_HALF_ULP * (ref.abs() + tol)
    if name == "h2" and key == "out":
        return tol + H2_REL * (ref.abs() + tol) + SPLIT_FLOOR / ops.A_SCALE_F16X3
    return tol


# ---------------------------------------------------------------------------------------------------------------------------------
# running one case through `impl` on views of NaN buffers
# ---------------------------------------------------------------------------------------------------------------------------------
def _block(dev, rows, cols, col0, extra, dtype):
    """A (rows, cols) block at row 1, column col0 of a NaN buffer of rows + 2 rows and a pitch >= cols + col0 + extra (a multiple of 8) -> (buffer, slices)."""
    buf = nans(dev, rows + 2, ops.round_up(cols + col0 + extra, 8), dtype=dtype)
    return buf, (slice(1, rows + 1), slice(col0, col0 + cols))


def _flat(dev, t, off, dtype=None):
    """`t` as a view `off` elements into a 1-D NaN buffer."""
    buf = nans(dev, t.numel() + 2 * off, dtype=dtype or t.dtype)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t.to(dev))
    return v


def run(impl, name, cs, entry="gemm", inp=None):
    """entry = "slab": the same call through `conv_slab`; inp: the operands (default: those of `inputs(name, cs)`).  -> {"out": (M, ncol) values, "tail": (M, n_store - N) raw zeros to be, "out_f32": (M, ncol), "out_t": (nbt, N - t_col0, t_rows)} in float64
    (only the requested ones), after the NaN-outside checks of every output buffer."""
    dev, dtype = dev_of(impl), DTYPES[name]
    td = torch.bfloat16 if name == "bf16" else torch.float32
    inp = inputs(name, cs) if inp is None else inp
    p = inp["packed"]
    tag = cs.tag(name)
    rows = cs.nb * cs.lin
    abuf, ablk = _block(dev, rows, cs.cp, A_COL0, 64 - A_COL0, td)
    abuf[ablk] = p["a"].to(dev)
    w = _flat(dev, p["w"], 64)
    bias = None if p["bias"] is None else _flat(dev, p["bias"], 4)
    slope = None if p["slope"] is None else _flat(dev, p["slope"], 4)
    res = None
    if p["res"] is not None:
        rbuf, rblk = _block(dev, cs.m, p["res"].shape[1], RES_COL0, 40, p["res"].dtype)
        rbuf[rblk] = p["res"].to(dev)
        res = rbuf[rblk]
    ncol = cs.ncol
    width = max(ncol, cs.n_store)
    w8 = ops.round_up(width, 8) if name == "h2" else width
    out = out_f = out_t = None
    if cs.outs in ("out", "both"):
        obuf, oblk = _block(dev, cs.m, w8, OUT_COL0, 24, td)
        out = obuf[oblk]
    if cs.outs in ("f32", "both"):
        fbuf, fblk = _block(dev, cs.m, ncol, F32_COL0, 16, torch.float32)
        out_f = fbuf[fblk]
    if cs.t_col0 is not None:
        nbt, nt, t_ld = cs.m // cs.t_rows, cs.n - cs.t_col0, ops.round_up(cs.t_rows, 32) + cs.t_pad
        tbuf = nans(dev, nbt * nt * t_ld + 64, dtype=td)
        out_t = tbuf[32:32 + nbt * nt * t_ld].view(nbt, nt, t_ld)
    if entry == "slab":
        assert cs.res_first and cs.outs == "out" and cs.stride == 1 and cs.lin == cs.lout and cs.n == cs.cp
        impl.conv_slab(dtype, abuf[ablk], w, bias, slope, res, out, nseq=cs.nb, l=cs.lout, taps=cs.taps, pad=cs.pad, w_scale=inp["ws"])
    else:
        impl.gemm(dtype, abuf[ablk], w, bias, slope, res, out, out_f, out_t, n=cs.n, cp=cs.cp, n_store=cs.n_store, t_col0=cs.t_col0 or 0, t_rows=cs.t_rows,
                  res_first=cs.res_first, taps=cs.taps, stride=cs.stride, pad=cs.pad, lin=cs.lin, lout=cs.lout, m=cs.m, w_scale=inp["ws"],
                  res_h2=cs.res == "h2")
    got = {}
    if out is not None:
        _nan_outside(tag + ".out", obuf, *oblk)
        o = got["raw_out"] = out.cpu()
        planes = [o]
        if name == "h2":
            planes = F.h2_planes(o.contiguous(), w8)
            o = (planes[0].double() + planes[1].double()) / ops.A_SCALE_F16X3
        z0, z1 = (ncol, w8) if name == "h2" else (cs.n, cs.n_store)       # H2: whole 8-column groups are stored, so also [max(N, n_store), w8)
        for t in planes:
            tail = t[:, z0:max(z0, z1)]
            assert bool(((tail == 0) & ~torch.signbit(tail)).all()), tag + f": the columns [{z0}, {z1}) of out are not exactly +0"
        got["out"] = o[:, :ncol].double()
    if out_f is not None:
        _nan_outside(tag + ".out_f32", fbuf, *fblk)
        got["out_f32"] = out_f.cpu().double()
    if out_t is not None:
        t = tbuf.cpu()
        assert bool(torch.isnan(t[:32]).all()) and bool(torch.isnan(t[32 + nbt * nt * t_ld:]).all()), tag + ": out_t written outside its batches"
        tv = out_t.cpu()
        assert bool(torch.isnan(tv[:, :, cs.t_rows:]).all()), tag + f": the columns [{cs.t_rows}, {t_ld}) of out_t lost their fill"
        got["out_t"] = tv[:, :, :cs.t_rows].double()
    return got


def to_t(v, cs):
    """(M, N) -> the transposed tail (nbt, N - t_col0, t_rows)."""
    return v[:, cs.t_col0:].reshape(cs.m // cs.t_rows, cs.t_rows, cs.n - cs.t_col0).permute(0, 2, 1)


@functools.lru_cache(maxsize=4)
def f32_restatement_error(name, cs):
    """The error of `fake_ops.gemm` with F32 on the CPU, on the operands of THIS case in dtype `name` (F16X3 / H2), against the float64 reference of
    the same values, per (row, column) -> (len(rows), N).  The stored values of a split dtype are the fp32 values that were packed, so A, W, bias and
    slope go over bit for bit; an H2 residual enters as the fp32 tensor of the values its image holds ((hi + lo) / 16, rounded to fp32 where the two
    planes span more than 24 bits: the restatement's reference takes the rounded value)."""
    inp = inputs(name, cs)
    c32 = dataclasses.replace(cs, res=None if cs.res is None else "f32", outs="f32", t_col0=None, t_rows=0, t_pad=0, n_store=0)
    f = lambda t: None if t is None else t.float()
    a, w, bias, slope, res = f(inp["a"]), f(inp["w"]), f(inp["bias"]), f(inp["slope"]), f(inp["res"])
    assert bool((a.double() == inp["a"]).all()) and bool((w.double() == inp["w"]).all())
    dbl = lambda t: None if t is None else t.double()
    inp32 = dict(a=inp["a"], w=inp["w"], bias=inp["bias"], slope=inp["slope"], res=dbl(res), ws=1.0,
                 packed=dict(a=a, w=w.reshape(cs.n, cs.taps * cs.cp), bias=bias, slope=slope, res=res))
    rows = sample_rows(cs.m) if cs.sample else torch.arange(cs.m)
    got = run(F, "f32", c32, inp=inp32)["out_f32"][rows]
    return (got - reference("f32", c32, rows, inp32)["ref"]).abs()


def check_gemm(impl, name, cs, wrong=True, entry="gemm"):
    """-> (max error, its fraction of the tolerance, and for F16X3 / H2 the two columns of the 4 x rule: fp32 restatement | impl)."""
    cs = cs.for_dtype(name)
    tag = cs.tag(name)
    got = run(impl, name, cs, entry)
    rows = sample_rows(cs.m) if cs.sample else torch.arange(cs.m)
    full = not cs.sample
    r = reference(name, cs, rows)
    ref, tol = r["ref"], r["tol"]
    inp = inputs(name, cs)
    worst, frac, four = 0.0, 0.0, None
    if name in SPLIT:
        e32 = f32_restatement_error(name, cs)
        tol4 = torch.maximum(4 * e32.amax(1, keepdim=True), 8 * EPS32 * r["s"]) + r["floors"]
        four = [float(e32.max()), 0.0]
    pieces = []
    for key in ("out", "out_f32"):
        if key in got:
            pieces.append((key, got[key][rows], ref[:, :cs.ncol], tol[:, :cs.ncol], (lambda t: t[:, :cs.ncol])))
    if "out_t" in got and cs.n > cs.t_col0:
        assert full
        pieces.append(("out_t", got["out_t"], to_t(ref, cs), to_t(tol, cs), (lambda t: to_t(t, cs))))
    for key, g, rf, tl, view in pieces:
        tl = format_tol(name, key, rf, tl)
        assert bool(torch.isfinite(g).all()), f"{tag}.{key}: not finite"
        e = _cmp(f"{tag}.{key}", g, rf, tl)
        fr = float(torch.nan_to_num((g - rf).abs() / tl, nan=0.0).max())
        worst, frac = max(worst, e), max(frac, fr)
        if name in SPLIT:
            t4 = format_tol(name, key, rf, view(tol4))
            err = (g - rf).abs()
            four[1] = max(four[1], float(err.max()))
            bad = int((~(err <= t4)).sum())
            print(f"{tag}.{key}: 4 x rule: fp32 restatement {four[0]:.3e} | kernel {float(err.max()):.3e}, worst fraction {float((err / t4).max()):.2f}")
            assert bad == 0, f"{tag}.{key}: {bad} entries outside 4 x the fp32 restatement's error (fraction {float((err / t4).max()):.2f})"
        if wrong and full:
            for label, wr in wrong_references(name, cs, inp, r, rows):
                sel = quiet_rows(cs, rows)
                gq, wq, tq = (g[sel], view(wr)[sel], tl[sel]) if key != "out_t" else (g, view(wr), tl)
                if key == "out_t" and (cs.kinds or cs.loud):
                    continue
                far_finite(f"{tag}.{key} vs {label}", gq, wq, tq)
            t_ld = ops.round_up(cs.t_rows, 32) + cs.t_pad
            if key == "out_t" and t_ld != cs.t_rows and rf.shape[0] * rf.shape[1] * cs.t_rows > t_ld:          # rows written with the pitch t_rows for t_ld, as far as they reach into the second row
                nbt, nt = rf.shape[:2]
                flat = torch.full((nbt * nt * t_ld,), float("nan"), dtype=torch.float64)
                flat[:nbt * nt * cs.t_rows] = rf.reshape(-1)
                far_finite(f"{tag}.out_t vs the pitch t_rows for t_ld", g, flat.view(nbt, nt, t_ld)[:, :, :cs.t_rows], tl)
    return worst, frac, four


def far_finite(name, got, wrong, tol):
    """`far` on the entries where the wrong reference is finite (it must have some): a NaN where a wrong reader would leave the data proves nothing."""
    ok = torch.isfinite(wrong)
    assert bool(ok.any()), name + ": the wrong reference has no finite entry"
    far(name, got[ok], wrong[ok], torch.as_tensor(tol, dtype=torch.float64).expand(wrong.shape)[ok])


def quiet_rows(cs, rows):
    """The output rows a wrong reference is judged on: the N(0,1) rows of a `kinds` case, the quiet sequence of a `loud` one, else all."""
    if cs.kinds:
        return rows % 5 == 0
    if cs.loud:
        return rows // cs.lout == cs.nb // 2
    return torch.ones(len(rows), dtype=torch.bool)


def wrong_references(name, cs, inp, r, rows):
    """(label, (len(rows), N) wrong reference) for every feature the case has."""
    out = []
    v, w2 = r["v"], r["w2"]
    ep = lambda vv=v, **kw: epilogue(vv, cs, inp, rows, **kw)[0]
    if cs.bias and cs.n > 1:
        out.append(("the bias of column n + 1", ep(bias_shift=1)))
    if cs.slope not in (None, 1.0):
        out.append(("the slope on the positive side", ep(slope_side="pos")))
    if cs.res is not None and cs.slope not in (None, 1.0):
        out.append(("the residual on the other side of the activation", ep(res_side=not cs.res_first)))
    if cs.res in ("lo", "f32") and cs.m > 1:
        flat = torch.cat([inp["res"].reshape(-1), inp["res"].reshape(-1)[:cs.m]])       # a pitch one element too long, running on into finite data
        out.append(("res read with another leading dimension", ep(res=torch.as_strided(flat, (cs.m, cs.n), (cs.n + 1, 1))[rows])))
    if cs.t_col0 is not None and cs.n > cs.t_col0 and cs.m // cs.t_rows > 1:
        nbt = cs.m // cs.t_rows
        out.append(("out_t rows of batch b + 1", r["ref"].reshape(nbt, cs.t_rows, cs.n).roll(-1, 0).reshape(cs.m, cs.n)))
    if not cs.identity:
        gx = lambda **kw: ep(gather(inp["a"], cs, rows, **kw).reshape(len(rows), -1) @ w2.t())
        pos = torch.arange(cs.lout)[:, None] * cs.stride + torch.arange(cs.taps)[None, :] - cs.pad
        if bool(((pos < 0) | (pos >= cs.lin)).any()):
            out.append(("no zero padding at a sequence edge", gx(edge="neighbour")))
        if cs.pad > 0:
            out.append(("pad off by one", gx(pad=cs.pad - 1)))
        if cs.stride > 1:
            out.append(("the stride ignored", gx(stride=1)))
        if cs.taps > 1 and cs.lin > 1:
            out.append(("the taps in reverse order", gx(reverse=True)))
        if cs.lin != cs.lout and cs.nb > 1:
            out.append(("Lin for Lout in the batch pitch", gx(pitch=cs.lin)))
    return out


def pad_only_rows(cs):
    """The output rows of a convolution case that see only padding."""
    pos = torch.arange(cs.lout)[:, None] * cs.stride + torch.arange(cs.taps)[None, :] - cs.pad
    dead = ~((pos >= 0) & (pos < cs.lin)).any(1)
    return dead.repeat(cs.nb)


# ---------------------------------------------------------------------------------------------------------------------------------
# table 6: `conv_slab`, the stride-1 C -> C convolution with the input slab in LDS (csrc/convslab.hip), 128 positions per block: against float64
# with the tolerances of `gemm` at the same geometry (taps, 1, pad, L, L), AND bit-identical to `gemm`
# ---------------------------------------------------------------------------------------------------------------------------------
SLAB_DTYPES = ("f32", "bf16", "f16x3")


def slab(c, taps, pad, nseq, l, res):
    return Case(m=nseq * l, n=c, cp=c, nb=nseq, lin=l, lout=l, taps=taps, stride=1, pad=pad, slope="vec", res="lo" if res else None, res_first=True,
                outs="out", loud=nseq == 3 and l > 1)


# every C, taps, pad in {0, taps // 2, taps - 1}, nseq, L around the 128-position block, with and without the shortcut
SLAB_CASES = [slab(64, 3, 0, 1, 1, True), slab(128, 3, 1, 3, 14, False), slab(64, 3, 2, 3, 127, True), slab(128, 15, 0, 1, 128, True),
              slab(64, 15, 7, 3, 129, False), slab(128, 15, 14, 1, 257, False), slab(64, 16, 0, 3, 257, True), slab(128, 16, 8, 3, 1, True),
              slab(64, 16, 15, 1, 14, False), slab(128, 3, 1, 1, 127, True), slab(64, 15, 7, 1, 128, True), slab(128, 16, 15, 3, 129, True)]
assert {c.lout for c in SLAB_CASES} == {1, 14, 127, 128, 129, 257} and {(c.taps, c.pad) for c in SLAB_CASES} >= {(t, p) for t in (3, 15, 16) for p in (0, t // 2, t - 1)}


def check_conv_slab(impl, name, cs):
    from forward_cases import bits_equal
    r = check_gemm(impl, name, cs, entry="slab")
    assert bits_equal(run(impl, name, cs, "slab")["raw_out"], run(impl, name, cs)["raw_out"]), cs.tag(name) + ": conv_slab and gemm differ in a bit"
    return r


# ---------------------------------------------------------------------------------------------------------------------------------
# table 6, `wav_conv_in` (csrc/wavconv.hip): the first layer on the raw waveform, one fmaf chain of `taps` terms per output in fp32:
#   out[(i B + b) Lout + l][c] = leaky(sum_k x_ib[l stride + k - pad] w[c][k] + bias[c], slope[c]),  x_ib = window i of clip b, zero outside [0, Lw)
# tol = taps u S (one rounding per fused multiply-add) + u (|v| + |bias|) + u |v s|; bf16 `out`: + 2^-8 relative
# ---------------------------------------------------------------------------------------------------------------------------------
WAV_DTYPES = ("f32", "bf16")
WAV_CLIPS, WAV_OUTSIDE = 2, 1e3
# (C, taps, stride, pad, Lw, nwin): every value of each at least once
WAV_CASES = [(8, 1, 1, 0, 100, 1), (64, 15, 5, 7, 1003, 2), (256, 16, 5, 1600, 100, 2), (8, 15, 5, 1600, 1003, 1), (64, 16, 1, 0, 1003, 1),
             (256, 1, 5, 7, 100, 2), (8, 16, 5, 7, 100, 1), (64, 1, 5, 1600, 100, 2), (256, 15, 1, 0, 100, 2)]


def check_wav_conv_in(impl, name, c, taps, stride, pad, lw, nwin):
    """Clips of pitch span + 25 inside a buffer of 1e3: the 5 samples in front of every clip's first window and the 20 behind its last one hold
    1e3 (the padding is the window's, not the clip's); two windows overlap by half.  -> (max error, its fraction of the tolerance)."""
    dev, dtype = dev_of(impl), DTYPES[name]
    td = torch.bfloat16 if name == "bf16" else torch.float32
    g = gen(zlib.crc32(repr((c, taps, stride, pad, lw, nwin)).encode()))
    hop = lw // 2 if nwin > 1 else 0
    span = (nwin - 1) * hop + lw
    lout = (lw + 2 * pad - taps) // stride + 1
    wbuf = torch.full((WAV_CLIPS, span + 25), WAV_OUTSIDE)
    wbuf[:, 5:5 + span] = _rn(g, WAV_CLIPS, span)
    w, bias = _rn(g, c, taps) / taps ** 0.5, _rn(g, c)
    slope = torch.cat([torch.full((c // 2,), 0.01), torch.ones(c - c // 2)])
    rows = nwin * WAV_CLIPS * lout
    obuf, oblk = _block(dev, rows, c, OUT_COL0, 24, td)
    tag = f"wav_conv_in[{name} C={c} taps={taps} stride={stride} pad={pad} Lw={lw} nwin={nwin}]"
    impl.wav_conv_in(dtype, wbuf.to(dev)[:, 5:], _flat(dev, w, 4), _flat(dev, bias, 4), _flat(dev, slope, 4), obuf[oblk], lout, stride, pad,
                     nwin=nwin, hop=hop, win_len=lw)
    _nan_outside(tag, obuf, *oblk)
    got = obuf[oblk].cpu().double().view(nwin, WAV_CLIPS, lout, c)

    def ref(window_padding=True, clip_major=False):
        pos = torch.arange(lout)[:, None] * stride + torch.arange(taps)[None, :] - pad                     # (Lout, taps), in window samples
        full = torch.nn.functional.pad(wbuf.double(), (pad + taps, pad + taps + stride * lout), value=WAV_OUTSIDE)
        out, s = [], []
        for i in range(nwin):
            x = full[:, (pad + taps + 5 + i * hop + pos).clamp(0, full.shape[1] - 1)]                        # (clips, Lout, taps)
            if window_padding:
                x = x * ((pos >= 0) & (pos < lw))
            out.append(x @ w.double().t())
            s.append(x.abs() @ w.double().abs().t())
        v, s = torch.stack(out), torch.stack(s)                                                            # (nwin, clips, Lout, C)
        if clip_major:
            v = v.transpose(0, 1).reshape(nwin, WAV_CLIPS, lout, c)
        t = v + bias.double()
        r = torch.where(t > 0, t, t * slope.double())
        return r, taps * EPS32 * s + EPS32 * (v.abs() + bias.double().abs() + r.abs())

    r, tol = ref()
    tol = format_tol(name, "out", r, tol)
    err = _cmp(tag, got, r, tol)
    frac = float(torch.nan_to_num((got - r).abs() / tol, nan=0.0).max())
    if pad > 0:
        far(tag + " vs the clip's samples as padding", got, ref(window_padding=False)[0], tol)
    if nwin > 1:
        far(tag + " vs output sequences ordered clip-major", got, ref(clip_major=True)[0], tol)
    return err, frac


# ---------------------------------------------------------------------------------------------------------------------------------
# table 6, `wav_block0` (csrc/convslab.hip): conv1 (15 taps, stride 5, pad 1600, folded BN, LeakyReLU 0.01) and the shortcut conv from the raw
# waveform, conv2 (15 taps, pad 7) on conv1's output, shortcut added before the second LeakyReLU.  Reference: that composite in float64 from the
# stored operands, nothing rounded between the layers.  A derived bound through two layers and a kink (an error of the first layer may flip the side
# of an activation of slope 0.01) would be loose, so the tolerance is the 4 x rule: 4 x the error of `fake_ops.wav_block0` in the same dtype on the CPU
# (its fp32 arithmetic with the mode's storage rounding between the layers), floor 8 EPS32 of the output scale
# ---------------------------------------------------------------------------------------------------------------------------------
BLOCK0_DTYPES = ("f32", "bf16", "f16x3")
BLOCK0_CASES = [(1, 1), (2, 2)]               # (nclip, nwin)
BLOCK0_LW, BLOCK0_C = 1000, 64


def _block0_run(impl, name, ops_in, nclip, nwin, hop, lout):
    dev, dtype = dev_of(impl), DTYPES[name]
    td = torch.bfloat16 if name == "bf16" else torch.float32
    wbuf, w1, b1, wds, bds, w2p, ws, b2, s2 = ops_in
    obuf, oblk = _block(dev, nwin * nclip * lout, BLOCK0_C, OUT_COL0, 24, td)
    impl.wav_block0(dtype, wbuf.to(dev)[:, 5:], w1.to(dev), _flat(dev, b1, 4), 0.01, wds.to(dev), _flat(dev, bds, 4), 5, 1600, _flat(dev, w2p, 64),
                    _flat(dev, b2, 4), _flat(dev, s2, 4), 15, 7, obuf[oblk], lout, nwin=nwin, hop=hop, win_len=BLOCK0_LW, w_scale=ws)
    _nan_outside(f"wav_block0[{name} nclip={nclip} nwin={nwin}]", obuf, *oblk)
    return obuf[oblk].cpu().double()


def check_wav_block0(impl, name, nclip, nwin):
    """-> (error of the fake_ops composite in the same dtype, error of `impl`), both against float64."""
    td = torch.bfloat16 if name == "bf16" else torch.float32
    c, lw = BLOCK0_C, BLOCK0_LW
    g = gen(100 * nclip + nwin)
    hop = lw // 2 if nwin > 1 else 0
    span = (nwin - 1) * hop + lw
    lout = (lw + 3200 - 15) // 5 + 1
    wbuf = torch.full((nclip, span + 25), WAV_OUTSIDE)
    wbuf[:, 5:5 + span] = _rn(g, nclip, span)
    w1, wds = _rn(g, c, 15) / 15 ** 0.5, _rn(g, c, 15) / 15 ** 0.5
    b1, bds, b2 = _rn(g, c), _rn(g, c), _rn(g, c)
    w2 = (_rn(g, c, 15, c) / (15 * c) ** 0.5).to(td)
    s2 = torch.full((c,), 0.01)
    w2p, ws = ops.split_f16_weights(w2.reshape(c, 15 * c)) if name == "f16x3" else (w2.reshape(c, 15 * c), 1.0)
    ops_in = (wbuf, w1, b1, wds, bds, w2p, ws, b2, s2)

    def ref(shortcut="before"):
        pos = torch.arange(lout)[:, None] * 5 + torch.arange(15)[None, :] - 1600
        inside = (pos >= 0) & (pos < lw)
        outs = []
        for i in range(nwin):
            x = wbuf.double()[:, (5 + i * hop + pos).clamp(0, wbuf.shape[1] - 1)] * inside                    # (clips, Lout, 15)
            y1 = x @ w1.double().t() + b1.double()
            y1 = torch.where(y1 > 0, y1, 0.01 * y1)
            sc = x @ wds.double().t() + bds.double()
            p2 = torch.arange(lout)[:, None] + torch.arange(15)[None, :] - 7
            x2 = y1[:, p2.clamp(0, lout - 1)] * ((p2 >= 0) & (p2 < lout))[:, :, None]                         # (clips, Lout, 15, C)
            v = torch.einsum("bltc,ntc->bln", x2, w2.double()) + b2.double()
            if shortcut == "before":
                v = v + sc
            v = torch.where(v > 0, v, 0.01 * v)
            if shortcut == "after":
                v = v + sc
            outs.append(v)
        return torch.stack(outs).reshape(nwin * nclip * lout, c)

    tag = f"wav_block0[{name} nclip={nclip} nwin={nwin}]"
    r = ref()
    e_fake = float((_block0_run(F, name, ops_in, nclip, nwin, hop, lout) - r).abs().max())
    got = _block0_run(impl, name, ops_in, nclip, nwin, hop, lout)
    tol = max(4 * e_fake, 8 * EPS32 * float(r.abs().max()))
    print(f"{tag}: fake_ops composite err {e_fake:.3e}")
    err = _cmp(tag, got, r, tol)
    far(tag + " vs no shortcut", got, ref(shortcut=None), tol)
    far(tag + " vs the shortcut behind the second activation", got, ref(shortcut="after"), tol)
    return e_fake, err
