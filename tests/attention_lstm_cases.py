"""The case table of the forward attention / LSTM-cell tests: the two kernel families that put a non-linearity behind an MFMA contraction
(csrc/attention.hip + attn_tile.h; EPI_LSTM of csrc/gemm_tile.h, csrc/lstm.hip, csrc/lstmseq.hip) and `softmax2_mix`, each against a float64
reference built from the stored operands, with the tolerance derived from the kernel's arithmetic next to each case and one plausible WRONG
reference per feature.

Every `check_*` takes `impl`: `pantomatrix_amd.ops` (tests/test_attention_lstm_gpu.py) or `tests/fake_ops.py` / another fp32 implementation on the
CPU (tests/test_attention_lstm_host.py).  Conventions as in tests/forward_cases.py: operands and outputs are offset, strided views of NaN-filled
buffers, outputs must still be NaN outside their block, every comparison goes through `_cmp` and prints its max error, a wrong reference must miss by
more than FAR x the tolerance, and what crosses the C ABI as `float` (the softmax scale) enters the reference with its fp32 value.

Rounding model used below (u = EPS32 = 2^-24):
  * an fp32 sum of n terms, in ANY order, is within (n - 1) u sum|terms| of the exact sum (Higham, Accuracy and Stability, 4.2): the MFMA
    accumulation order never enters a bound;
  * split-f16 (EMAGE_F16X3 / EMAGE_H2): x s = hi + lo + r with hi = rne_f16(x s), lo = rne_f16(x s - hi): |r| <= 2^-22 |x s|, or <= 2^-25 where
    lo is an fp16 subnormal (spacing 2^-24).  A product x y is taken as hi hi + hi lo + lo hi (exact fp16 products, fp32 accumulate): it misses x y
    by the two residuals and the dropped lo lo <= 2^-22 |x y|:   3 2^-22 |x y| + (2^-25 / s_x) |y| + (2^-25 / s_y) |x|,
    and the contraction sums 3 n such terms: (3 n) u sum|x y| on top.
The any-order accumulation bound is a worst case: fp32-grade results sit at a few percent of the attention tolerances, so a defect that costs one
order of magnitude on N(0,1) inputs (a dropped low-plane MFMA, say) lands near the bound, not clearly outside it.  For N(0,1) inputs the older
fixed-tolerance tests stay the tighter check (tests/test_kernels_gpu.py::test_attention at 2e-5, tests/test_lstm_gpu.py at 2e-5); what these cases
add is the peaked / shifted / padded / saturated inputs, the boundary shapes, the independent float64 references and the wrong references."""
import functools
import math
import types

import torch

import fake_ops as F
from forward_cases import dev_of, far, gen, nans
from kernel_checks import EPS32, SPLIT_FLOOR, SPLIT_REL, _cmp, _nan_outside
from pantomatrix_amd import ops
from pantomatrix_amd._lib import BF16, F32, F16X3, H2
from pantomatrix_amd.modeling_lstm_audio import _LstmAudioModel

BF16_HALF_ULP = 2.0 ** -8           # unit roundoff of 8 significant bits (round to nearest): half an ulp, relative

# ---------------------------------------------------------------------------------------------------------------------------------
# attention / attention_dropout: one wave per 16-query tile, 4 tiles per workgroup; NT = 2 / 4 / 8 key tiles for Tk <= 32 / 64 / 128;
# split-f16 with Tk <= 64 stages K / V^T in LDS, everything else reads them through buffer descriptors
# ---------------------------------------------------------------------------------------------------------------------------------
HD = 192
ATT_SCALE = float(1.0 / torch.sqrt(torch.tensor(float(HD))))        # 1.0f / sqrtf(192.0f): the kernel's own fp32 constant
ATT_DTYPES = {"f32": F32, "bf16": BF16, "f16x3": F16X3, "h2": H2}
VT_PAD = 1e3                       # EVERY case holds this in the V^T columns [Tk, ldvt), not 0: finite, as the contract asks, and large
PEAK_MARGIN = 40.0
ATT_TK = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 80, 96, 97, 127, 128)
ATT_TQ = (1, 15, 16, 17, 63, 64, 65, 130)
# (Tk, Tq, B, H, kind): every Tk and every Tq at least once, every kind at a ragged Tk (< 16 NT) and at a full one (32, 64, 128)
ATT_BASE = [
    (1, 17, 1, 3, "normal"),       # one key: the output is the V row
    (15, 1, 2, 1, "peaked"),       # one query, 15 surplus lanes in the tile
    (16, 15, 1, 1, "shifted"),
    (17, 16, 2, 3, "qzero"),
    (31, 63, 1, 1, "normal"),
    (32, 64, 1, 3, "peaked"),      # full NT = 2: no key mask; four full query tiles
    (33, 65, 2, 1, "shifted"),     # NT = 4 by one key; a second workgroup with one live wave
    (63, 130, 1, 1, "qzero"),      # three workgroups per (batch, head), Tq > Tk
    (64, 17, 1, 3, "normal"),      # the inference window's Tk; last size of the LDS-staged split-f16 path
    (64, 63, 1, 1, "shifted"),
    (65, 16, 1, 1, "peaked"),      # first size of the register path, NT = 8, ldvt = 96 < 16 NT
    (80, 1, 2, 1, "normal"),       # ldvt = 96 with 16 padding columns
    (96, 65, 1, 1, "shifted"),     # ldvt = 96 = Tk: ragged for the mask, no padding column
    (97, 15, 1, 3, "qzero"),
    (127, 64, 1, 1, "peaked"),
    (128, 130, 1, 1, "normal"),    # full NT = 8, Tq > the largest Tk
    (128, 17, 1, 1, "peaked"),
    (128, 16, 1, 1, "qzero"),
    (32, 16, 1, 1, "qzero"),
]
ATT_CASES = [(name,) + row for name in ATT_DTYPES for row in ATT_BASE]
# the V^T rows behind the last head are NaN in every case, so under the other answer to "may a V^T chunk be read past ldvt" (a documented
# finite-neighbour contract instead of the zero operand the NT = 8 path now takes) every Tk in 65..96 gives NaN; this one is named for it
ATT_READS_PAST_LDVT = ("f32", 80, 1, 2, 1, "normal")
DROP_DTYPES = ("f32", "f16x3")
DROP_BASE = [(15, 17, 2, 3), (33, 16, 1, 1), (65, 15, 1, 1), (127, 17, 1, 1), (32, 64, 1, 1), (64, 65, 1, 3), (128, 16, 2, 1)]      # (Tk, Tq, B, H)
DROP_CASES = [(name,) + row for name in DROP_DTYPES for row in DROP_BASE]
DROP_P = 0.1
assert {c[1] for c in ATT_CASES} == set(ATT_TK) and {c[2] for c in ATT_CASES} == set(ATT_TQ)


def worst_fraction(got, ref, tol):
    """The largest error / tolerance over the entries (an exact entry under a zero tolerance counts as 0)."""
    return float(torch.nan_to_num((got - ref).abs() / tol, nan=0.0).max())


def att_nt(tk):
    return 2 if tk <= 32 else 4 if tk <= 64 else 8


def att_inputs(name, tk, tq, b, h, kind):
    """-> q (B, Tq, H, hd), k, v (B, Tk, H, hd) as STORED (bf16-rounded for BF16) in float64, and for `peaked` the winning key (B, H, Tq).
      normal   N(0,1)
      peaked   q = 6 k_t: the score of key t is 6 |k_t|^2 / sqrt(192) ~ 83, of the others 6 k_t.k_j / sqrt(192) ~ N(0, 6^2); t = Tk - 1 for queries
               0 mod 3, key 0 for 1 mod 3, seeded for the rest
      shifted  q, k = 4.65 e + 0.5 N(0,1) with a sign vector e: scores 300 +- 3 (192 x 4.65^2 / sqrt(192)), |x| < 8 << 4094
      qzero    q = 0"""
    g = gen(100000 * tk + 100 * tq + 10 * b + h + len(name) + 7 * len(kind))
    q, k, v = torch.randn(b, tq, h, HD, generator=g), torch.randn(b, tk, h, HD, generator=g), torch.randn(b, tk, h, HD, generator=g)
    target = None
    if kind == "peaked":
        target = torch.randint(0, tk, (b, h, tq), generator=g)
        i = torch.arange(tq)
        target[:, :, i % 3 == 0] = tk - 1
        target[:, :, i % 3 == 1] = 0
        kt = k.permute(0, 2, 1, 3).gather(2, target.unsqueeze(-1).expand(b, h, tq, HD))          # (B, H, Tq, hd)
        q = 6.0 * kt.permute(0, 2, 1, 3)
    elif kind == "shifted":
        e = torch.where(torch.rand(HD, generator=g) < 0.5, -1.0, 1.0)
        q, k = 4.65 * e + 0.5 * q, 4.65 * e + 0.5 * k
    elif kind == "qzero":
        q = torch.zeros_like(q)
    td = torch.bfloat16 if name == "bf16" else torch.float32
    return tuple(t.to(td).double() for t in (q, k, v)) + (target,)


def att_ref(q, k, v, pmask=None, *, scale=ATT_SCALE, pad=0, renorm=False, next_head=False):
    """float64 softmax(q k^T scale) v per (batch, head) from the stored operands -> (o (B, Tq, H, hd), s, p (B, H, Tq, Tk)).  The wrong variants:
    scale = 1; `pad` further keys scored 0 that carry VT_PAD; the dropout mask applied BEFORE the normalisation; V of the next head."""
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * scale
    vv = v.roll(-1, 2) if next_head else v
    if pad:
        s = torch.cat([s, torch.zeros(s.shape[:3] + (pad,), dtype=s.dtype)], -1)
        vv = torch.cat([vv, torch.full((v.shape[0], pad) + v.shape[2:], VT_PAD, dtype=v.dtype)], 1)
    if renorm:
        e = torch.exp(s - s.amax(-1, keepdim=True)) * pmask
        p = e / e.sum(-1, keepdim=True).clamp_min(1e-300)
    else:
        p = torch.softmax(s, -1)
        if pmask is not None:
            p = p * pmask
    return torch.einsum("bhqk,bkhd->bqhd", p, vv), s, p


def att_tol(name, q, k, v, s, p, o, dropout=False):
    """Per output entry, first order, u = EPS32:
      score     ds = c_qk scale sum_i |q_i k_i| + 2 u |s|                       (the product with the fp32 scale, and that constant's own rounding)
                c_qk = hd u for the fp32 / bf16 MFMA (exact bf16 products); split-f16: 3 2^-22 + 3 hd u, and the low planes' floor at the operand
                scale 16:  2^-29 scale (sum|q_i| + sum|k_i|)
      softmax   p_j = e^(s_j - max) / sum: a score error of at most ds_row = max_j ds moves every p_j by the factor e^(+-2 ds_row); then
                u |s_j - max| (the subtraction; BF16: twice, __expf multiplies by log2 e first) + 2 u (exp within an ulp) + (Tk - 1) u (the sum of Tk
                positive terms) + 2 u (1 / sum, e * inv); BF16: + 2^-8 (p rounded to 8 bits); dropout: + u (p * mask).  Absolute floor 1e-37 (exp
                flushing to 0 below e^-87)
      output    sum_j dp_j |v_j| + c_pv sum_j p_j |v_j|, c_pv = (16 NT) u (the P V contraction runs over all 16 NT key slots); split-f16:
                3 2^-22 + 3 (16 NT) u, and the floors of P (scale 1024) and V (scale 16):  2^-35 sum_j |v_j| + 2^-29 sum_j p_j
      storage   BF16: + 2^-8 |o|; H2 image (scale 16, decoded as (hi + lo) / 16 in fp32): + (2^-22 + u) |o| + 2^-29"""
    split = name in ("f16x3", "h2")
    tk = k.shape[1]
    nkeys = 16 * att_nt(tk)
    qa, ka, va = q.abs(), k.abs(), v.abs()
    sabs = torch.einsum("bqhd,bkhd->bhqk", qa, ka) * ATT_SCALE
    if split:
        ds = (SPLIT_REL + 3 * HD * EPS32) * sabs \
            + SPLIT_FLOOR / 16 * ATT_SCALE * (qa.sum(-1).permute(0, 2, 1).unsqueeze(-1) + ka.sum(-1).permute(0, 2, 1).unsqueeze(-2))
    else:
        ds = HD * EPS32 * sabs
    ds = ds + 2 * EPS32 * s.abs()
    gap = (s - s.amax(-1, keepdim=True)).abs()
    rel = 2 * ds.amax(-1, keepdim=True) + EPS32 * ((2 if name == "bf16" else 1) * gap + tk + 3 + (1 if dropout else 0))
    if name == "bf16":
        rel = rel + BF16_HALF_ULP
    dp = p * rel + 1e-37
    pv = torch.einsum("bhqk,bkhd->bqhd", p, va)
    tol = torch.einsum("bhqk,bkhd->bqhd", dp, va)
    if split:
        tol = tol + (SPLIT_REL + 3 * nkeys * EPS32) * pv + SPLIT_FLOOR / 1024 * va.sum(1, keepdim=True) + SPLIT_FLOOR / 16 * p.sum(-1).permute(0, 2, 1).unsqueeze(-1)
    else:
        tol = tol + nkeys * EPS32 * pv
    if name == "bf16":
        tol = tol + BF16_HALF_ULP * o.abs()
    if name == "h2":
        tol = tol + (2.0 ** -22 + EPS32) * o.abs() + SPLIT_FLOOR / 16
    return tol


def att_run(impl, tag, name, q, k, v, pmask=None):
    """q / k / out: rows [1, 1 + B T) and a column block of (B T + 2, H hd + 64) NaN buffers (three different column offsets); V^T: rows
    [8, 8 + H hd) of a (B, H hd + 24, ldvt) NaN buffer, columns [Tk, ldvt) = VT_PAD.  -> the output (B, Tq, H, hd) in float64."""
    dev, dtype = dev_of(impl), ATT_DTYPES[name]
    td = torch.bfloat16 if name == "bf16" else torch.float32
    b, tq, h, _ = q.shape
    tk = k.shape[1]
    d, ldvt, r0 = h * HD, ops.round_up(tk, 32), 8
    ld, rows = d + 64, d + 24
    qb, kb, ob = nans(dev, b * tq + 2, ld, dtype=td), nans(dev, b * tk + 2, ld, dtype=td), nans(dev, b * tq + 2, ld, dtype=td)
    qblk, kblk, oblk = (slice(1, b * tq + 1), slice(32, 32 + d)), (slice(1, b * tk + 1), slice(16, 16 + d)), (slice(1, b * tq + 1), slice(48, 48 + d))
    qb[qblk], kb[kblk] = q.reshape(b * tq, d).to(td).to(dev), k.reshape(b * tk, d).to(td).to(dev)
    vb = nans(dev, b, rows, ldvt, dtype=td)
    vb[:, r0:r0 + d, :tk] = v.permute(0, 2, 3, 1).reshape(b, d, tk).to(td).to(dev)
    vb[:, r0:r0 + d, tk:] = VT_PAD
    if pmask is None:
        impl.attention(dtype, qb[qblk], kb[kblk], vb[:, r0:], rows, ob[oblk], b, h, tq, tk, HD)
    else:
        impl.attention_dropout(dtype, qb[qblk], kb[kblk], vb[:, r0:], rows, ob[oblk], b, h, tq, tk, HD, pmask.float().contiguous().to(dev))
    _nan_outside(tag, ob, *oblk)
    got = ob[oblk].cpu()
    if name == "h2":                     # the image as test_attention_h2_output_equals_f16x3 reads it: 32-byte groups [8 hi | 8 lo] of 16 x
        got = F.h2_values(got.contiguous(), d)
    return got.double().view(b, tq, h, HD)


def peak_margin(s, target):
    """The smallest float64 score margin of the winning key over every other key."""
    win = s.gather(-1, target.unsqueeze(-1))
    rest = s.scatter(-1, target.unsqueeze(-1), -math.inf)
    return float((win - rest.amax(-1, keepdim=True)).min())


def check_attention(impl, name, tk, tq, b, h, kind):
    """-> (max error, its fraction of the tolerance at that entry)."""
    q, k, v, target = att_inputs(name, tk, tq, b, h, kind)
    tag = f"attention[{name} B={b} H={h} Tq={tq} Tk={tk} {kind}]"
    got = att_run(impl, tag, name, q, k, v)
    ref, s, p = att_ref(q, k, v)
    tol = att_tol(name, q, k, v, s, p, ref)
    assert bool(torch.isfinite(got).all()), tag + ": not finite"
    err = _cmp(tag, got, ref, tol)
    frac = worst_fraction(got, ref, tol)
    ldvt = ops.round_up(tk, 32)
    if kind == "peaked":
        m = peak_margin(s, target)
        print(f"{tag}: float64 score margin {m:.1f}")
        assert m >= PEAK_MARGIN, (tag, m)
        rows = v.permute(0, 2, 1, 3).gather(2, target.unsqueeze(-1).expand(b, h, tq, HD)).permute(0, 2, 1, 3)
        _cmp(tag + " vs the winning V row", got, rows, tol + tk * math.exp(-PEAK_MARGIN) * 2 * float(v.abs().max()))
    if kind == "qzero":
        _cmp(tag + " vs the mean of the V rows", got, v.mean(1, keepdim=True).expand_as(got), tol)
    if kind == "shifted":
        assert float(s.amax(-1).min()) > 2 * math.log(3.4e38), tag + ": the row maximum is not far above log(FLT_MAX)"
        e = torch.exp(s.float())                                          # fp32 without the max subtraction: inf / inf
        far(tag + " vs no max subtraction", got, torch.einsum("bhqk,bkhd->bqhd", (e / e.sum(-1, keepdim=True)).double(), v), tol)
    if kind == "normal" and tk > 1:          # one key: p = 1 whatever the scores
        far(tag + " vs no 1 / sqrt(hd)", got, att_ref(q, k, v, scale=1.0)[0], tol)
    if kind in ("normal", "qzero") and ldvt > tk:
        far(tag + " vs padded keys scored 0", got, att_ref(q, k, v, pad=ldvt - tk)[0], tol)
    if h > 1:
        far(tag + " vs V of the next head", got, att_ref(q, k, v, next_head=True)[0], tol)
    return err, frac


def check_attention_dropout(impl, name, tk, tq, b, h):
    """N(0,1) operands, mask = Bernoulli(0.9) / 0.9 as fp32; query row 1 of every (batch, head) all zero, row 2 all ones."""
    q, k, v, _ = att_inputs(name, tk, tq, b, h, "normal")
    g = gen(77 * tk + tq)
    pmask = ((torch.rand(b, h, tq, tk, generator=g) >= DROP_P).float() / torch.tensor(1 - DROP_P, dtype=torch.float32)).double()
    pmask[:, :, 1], pmask[:, :, 2] = 0.0, 1.0
    tag = f"attention_dropout[{name} B={b} H={h} Tq={tq} Tk={tk}]"
    got = att_run(impl, tag, name, q, k, v, pmask)
    ref, s, p = att_ref(q, k, v, pmask)
    tol = att_tol(name, q, k, v, s, p, ref, dropout=True)
    err = _cmp(tag, got, ref, tol)
    frac = worst_fraction(got, ref, tol)
    assert bool((got[:, 1] == 0).all()), tag + ": an all-zero mask row gives exactly 0"
    plain, s0, p0 = att_ref(q, k, v)
    _cmp(tag + " all-ones row vs plain attention", got[:, 2], plain[:, 2], att_tol(name, q, k, v, s0, p0, plain, dropout=True)[:, 2])
    far(tag + " vs the mask before the normalisation", got, att_ref(q, k, v, pmask, renorm=True)[0], tol)
    far(tag + " vs no 1 / sqrt(hd)", got, att_ref(q, k, v, pmask, scale=1.0)[0], tol)
    if h > 1:
        far(tag + " vs V of the next head", got, att_ref(q, k, v, pmask, next_head=True)[0], tol)
    return err, frac


def vt_chunk_columns(name, tk):
    """Index arithmetic of attn_tile.h's register path (`load_v`): the V^T columns chunk c of lane group fg covers, for every (c, fg) -> list of
    (c, first column, last column).  fp32: chunk c = 4 floats at 16 c + 4 fg, c < NT.  bf16: 4 + 4 values at 32 c + 4 fg and 32 c + 16 + 4 fg,
    c < (NT + 1) / 2."""
    nt = att_nt(tk)
    if name == "bf16":
        return [(c, 32 * c, 32 * c + 16 + 4 * 3 + 3) for c in range((nt + 1) // 2)]
    return [(c, 16 * c, 16 * c + 4 * 3 + 3) for c in range(nt)]


def vt_chunk_is_loaded(name, tk, c, ldvt):
    """The kernel's condition: on the NT = 8 path a chunk whose first column lies at or past ldvt is a zero operand."""
    kpc = 32 if name == "bf16" else 16
    return not (att_nt(tk) == 8 and c * kpc >= 96 and c * kpc >= ldvt)


# ---------------------------------------------------------------------------------------------------------------------------------
# LSTM cell: lstm_step / lstm_step_pair (64 x 64 GEMM tiles with the cell in the epilogue), lstm_layer (persistent recurrence)
# ---------------------------------------------------------------------------------------------------------------------------------
LSTM_DTYPES = {"f32": F32, "f16x3": F16X3}
LSTM_B = (1, 63, 64, 65, 130)
LSTM_H = (64, 256, 512)
# (dtype, B, H, paired): every B x H through lstm_step (two launches per step) AND through lstm_step_pair (both directions in one launch)
LSTM_STEP_CASES = [(name, b, hid, paired) for name in LSTM_DTYPES for b in LSTM_B for hid in LSTM_H for paired in (False, True)]
LSTM_KINDS = ("N(0,1)", "1e-4 N(0,1)", "+-30", "+-100", "+-1e4", "forget gate open, |c0| = 20", "c0 = 0")
# absolute error of one non-linearity.  FAST = false: expf / tanhf within an ulp (2 u relative), 1 + e and the division one rounding each, values
# <= 1: 4 u.  FAST = true (split-f16): sigmoid = rcp(1 + exp2(-c x)): the fp32 constant c and the product c x carry 2 u |c x| into the exponent, i.e.
# 2 |x| u relative into e = exp2(.), exp2 and rcp are within an ulp, 1 + e rounds once:  |d sigmoid| <= s (1 - s) (2 |x| + 2) u + 3 u s <=
# (0.45 + 0.5 + 3) u <= 4 u  (x s (1 - s) <= 0.224);  tanh = 1 - 2 r, r = sigmoid(-2 x): 2 x 4 u + u (the subtraction) = 9 u: ABSOLUTE, so at
# |x| = 1e-4 three digits are left
NL_SIGMOID = {"f32": 4 * EPS32, "f16x3": 4 * EPS32}
NL_TANH = {"f32": 4 * EPS32, "f16x3": 9 * EPS32}


class _Pack:
    """What `_LstmAudioModel._pack_lstm` needs of the product's weight packer, with `_pack_mat` the identity: the regrouped matrices stay readable.
    Relies on that method's internals: it reads `pk.p[<state-dict key>]`, `pk.dt`, calls `pk._pack_mat(w) -> (operand, padded K, w_scale)`, writes
    `pk.w["<name>.hh.<layer>.<dir>"]["w"]` and `pk.w["<name>.ih.<layer>"]["w" / "b"]`, and reads `self.config.hidden_size` and
    `self.h2_input_projection`; tests/test_attention_lstm_host.py::test_product_regroup_is_a_permutation pins what comes out."""

    def __init__(self, p):
        self.p, self.w, self.dt, self.device = p, {}, F32, "cpu"

    def _pack_mat(self, w):
        return w, w.shape[1], 1.0


def product_regroup(w_hh):
    """The two directions' weight_hh (4H, H) in torch's layout -> ([regrouped weight_hh per direction], idx (8H,)) through the PRODUCT's own
    regrouping: `_pack_lstm` is run on an nn.LSTM state dict whose weight_ih is the identity and whose biases are zero, so the stacked input
    projection it packs is the selection matrix of gates_x:  gates_x[..., n] = torch-layout gates of direction n // 4H at column idx[n]."""
    hid = w_hh[0].shape[1]
    p = {}
    for w, sfx in zip(w_hh, ("", "_reverse")):
        p[f"lstm.weight_hh_l0{sfx}"], p[f"lstm.weight_ih_l0{sfx}"] = w, torch.eye(4 * hid)
        p[f"lstm.bias_ih_l0{sfx}"] = p[f"lstm.bias_hh_l0{sfx}"] = torch.zeros(4 * hid)
    pk = _Pack(p)
    _LstmAudioModel._pack_lstm(types.SimpleNamespace(config=types.SimpleNamespace(hidden_size=hid), h2_input_projection=False), pk, "lstm", 1)
    sel = pk.w["lstm.ih.0"]["w"]
    assert sel.shape == (8 * hid, 4 * hid) and bool(((sel == 0) | (sel == 1)).all()) and bool((sel.sum(1) == 1).all())
    assert not bool(pk.w["lstm.ih.0"]["b"].any())
    return [pk.w["lstm.hh.0.0"]["w"], pk.w["lstm.hh.0.1"]["w"]], sel.argmax(1)


def to_product_gates(gates, idx):
    """gates (2, ..., 4H) in torch's layout [i | f | g | o] -> (..., 8H) as `gates_x` holds them."""
    n = gates.shape[-1]
    return torch.cat([gates[0][..., idx[:n]], gates[1][..., idx[n:]]], -1)


def pack_w(name, w, dev):
    """-> (operand, w_scale) of a regrouped weight_hh for the dtype."""
    if name == "f16x3":
        p, s = ops.split_f16_weights(w)
        return p.to(dev), s
    return w.to(dev), 1.0


def cell64(gates, h, c, w, order="ifgo", cell_sigmoid=False):
    """The cell of torch's nn.LSTM documentation, written out, in float64 and in torch's layout:
        i = sigmoid(W_ii x + b_ii + W_hi h + b_hi) ... g = tanh(.), c' = f c + i g, h' = o tanh(c');  `gates` is the x part with both biases.
    Wrong variants: the gate blocks read as i, f, o, g; sigmoid on the cell gate."""
    a = gates + h @ w.t()
    i, f, g, o = a.chunk(4, -1)
    if order == "ifog":
        g, o = o, g
    gg = torch.sigmoid(g) if cell_sigmoid else torch.tanh(g)
    cn = torch.sigmoid(f) * c + torch.sigmoid(i) * gg
    return torch.sigmoid(o) * torch.tanh(cn), cn


def cell_tol(name, gates, h, c, w, ws, dh, dc):
    """First-order error bound of one step (u = EPS32) given the bounds dh, dc of the incoming state -> (dh', dc').
      pre-activation  da = c_hw sum_k |h_k w_k| + u |a| (adding gates_x) + sum_k |w_k| dh_k
                      c_hw = H u (fp32 MFMA); split-f16: 3 2^-22 + 3 H u, and the floors  2^-29 sum|w_k| (h at scale 16) + (2^-25 / w_scale) sum|h_k|
      gates           d sigmoid = s (1 - s) da + NL_SIGMOID,  d tanh = (1 - t^2) da + NL_TANH
      cell            dc' = |c| d f + f dc + |g| d i + i d g + 2 u (|f c| + |i g|)           (the products and the sum; the |c| d f term is what a
                      large cell state behind an open forget gate pays)
      output          dh' = |tanh c'| d o + o ((1 - tanh^2 c') dc' + NL_TANH) + u |h'|"""
    hid = h.shape[-1]
    hw = h.abs() @ w.abs().t()
    if name == "f16x3":
        da = (SPLIT_REL + 3 * hid * EPS32) * hw + SPLIT_FLOOR / 16 * w.abs().sum(1) + SPLIT_FLOOR / ws * h.abs().sum(-1, keepdim=True)
    else:
        da = hid * EPS32 * hw
    a = gates + h @ w.t()
    da = da + EPS32 * a.abs() + dh @ w.abs().t()
    (i, f, g, o), (dai, daf, dag, dao) = a.chunk(4, -1), da.chunk(4, -1)
    si, sf, so, tg = torch.sigmoid(i), torch.sigmoid(f), torch.sigmoid(o), torch.tanh(g)
    nls, nlt = NL_SIGMOID[name], NL_TANH[name]
    dsi, dsf, dso = si * (1 - si) * dai + nls, sf * (1 - sf) * daf + nls, so * (1 - so) * dao + nls
    dtg = (1 - tg ** 2) * dag + nlt
    cn = sf * c + si * tg
    dcn = c.abs() * dsf + sf * dc + tg.abs() * dsi + si * dtg + 2 * EPS32 * ((sf * c).abs() + (si * tg).abs())
    tc = torch.tanh(cn)
    dhn = tc.abs() * dso + so * ((1 - tc ** 2) * dcn + nlt) + EPS32 * (so * tc).abs()
    return dhn, dcn


LSTM_T = 3      # time slots of the (B, T, .) tensors the two steps are views of


def lstm_step_inputs(b, hid):
    """Torch layout, both directions: w (4H, H) ~ N(0, 1 / H); gates (2, B, T, 4H); h0, c0 (2, B, H).  Row kinds by (row + B) % 7, see LSTM_KINDS:
    rows of kind 1 also start from h0 = 0, so the first step's pre-activation is the 1e-4-scaled gates_x exactly."""
    g = gen(1000 * b + hid)
    w = [torch.randn(4 * hid, hid, generator=g) / hid ** 0.5 for _ in range(2)]
    gates = torch.randn(2, b, LSTM_T, 4 * hid, generator=g)
    sign = torch.where(torch.rand(2, b, LSTM_T, 4 * hid, generator=g) < 0.5, -1.0, 1.0)
    kind = (torch.arange(b) + b) % 7
    gates[:, kind == 1] *= 1e-4
    for kd, mag in ((2, 30.0), (3, 100.0), (4, 1e4)):
        gates[:, kind == kd] = mag * sign[:, kind == kd]
    gates[:, kind == 5, :, hid:2 * hid] = 30.0
    c0 = 0.5 * torch.randn(2, b, hid, generator=g)
    c0[:, kind == 5] = 20.0 * sign[:, kind == 5, 0, :hid]
    c0[:, kind == 6] = 0.0
    h0 = torch.tanh(torch.randn(2, b, hid, generator=g))
    h0[:, kind == 1] = 0.0
    return w, gates, h0, c0, kind


def check_lstm_steps(impl, name, b, hid, paired):
    """Two consecutive steps of both directions (forward at time slots 0, 1; backward at T - 1, T - 2) on strided views: h_out the column halves
    of a NaN (B, T, 2H + 32) buffer's block, gates_x the halves of a (B, T, 8H) tensor whose unused slots are NaN, h0 / c0 views of padded NaN
    buffers.  `paired`: through lstm_step_pair, else one lstm_step per direction.  -> {"h": (err, frac), "c": (err, frac)}."""
    dev, dtype = dev_of(impl), LSTM_DTYPES[name]
    w, gates, h0, c0, kind = lstm_step_inputs(b, hid)
    wp, idx = product_regroup(w)
    packed = [pack_w(name, m, dev) for m in wp]
    slots = ((0, 1), (LSTM_T - 1, LSTM_T - 2))
    gx = to_product_gates(gates, idx)
    gx[:, slots[0][1] + 1:, :4 * hid] = float("nan")
    gx[:, :slots[1][1], 4 * hid:] = float("nan")
    gxd = gx.to(dev)
    hbuf, cbuf, h0buf = nans(dev, b, LSTM_T, 2 * hid + 32), nans(dev, 2, b + 2, hid + 4), nans(dev, 2, b + 1, hid + 8)
    cv, h0v = cbuf[:, 1:b + 1, 2:2 + hid], h0buf[:, 1:, 4:4 + hid]
    cv.copy_(c0.to(dev))
    h0v.copy_(h0.to(dev))
    hout = lambda d, s: hbuf[:, s, 16 + d * hid:16 + (d + 1) * hid]
    prev = [h0v[0], h0v[1]]
    for step in range(2):
        args = [(prev[d], packed[d][0], gxd[:, slots[d][step], 4 * hid * d:4 * hid * (d + 1)], cv[d], hout(d, slots[d][step]), packed[d][1]) for d in range(2)]
        if paired:
            impl.lstm_step_pair(dtype, args[0], args[1])
        else:
            for hp, wm, gt, cs, ho, sc in args:
                impl.lstm_step(dtype, hp, wm, gt, cs, ho, w_scale=sc)
        prev = [a[4] for a in args]
    tag = f"lstm_step{'_pair' if paired else ''}[{name} B={b} H={hid}]"
    written = torch.zeros(b, LSTM_T, 2 * hid + 32, dtype=torch.bool)
    for d in range(2):
        for s in slots[d]:
            written[:, s, 16 + d * hid:16 + (d + 1) * hid] = True
    hb = hbuf.cpu()
    assert bool(torch.isnan(hb[~written]).all()), tag + ": h written outside the two steps' blocks"
    _nan_outside(tag + ".c", cbuf, slice(None), slice(1, b + 1), slice(2, 2 + hid))
    out = {}
    for d in range(2):
        wd = w[d].double()
        refs = {}
        for variant, kw in (("", {}), (" vs gate order i, f, o, g", dict(order="ifog")), (" vs sigmoid on the cell gate", dict(cell_sigmoid=True))):
            h, c, hs = h0[d].double(), c0[d].double(), []
            for step in range(2):
                h, c = cell64(gates[d][:, slots[d][step]].double(), h, c, wd, **kw)
                hs.append(h)
            refs[variant] = (hs, c)
        h, c = cell64(gates[d][:, slots[d][0]].double(), h0[d].double(), c0[d].double(), wd)
        refs[" vs the cell state not carried"] = ([h, cell64(gates[d][:, slots[d][1]].double(), h, torch.zeros_like(c), wd)[0]], None)
        dh, dc, tols = torch.zeros(b, hid, dtype=torch.float64), torch.zeros(b, hid, dtype=torch.float64), []
        h, c = h0[d].double(), c0[d].double()
        for step in range(2):
            gt = gates[d][:, slots[d][step]].double()
            dh, dc = cell_tol(name, gt, h, c, wd, packed[d][1], dh, dc)
            h, c = cell64(gt, h, c, wd)
            tols.append(dh)
        got_h = [hb[:, slots[d][step], 16 + d * hid:16 + (d + 1) * hid].double() for step in range(2)]
        got_c = cv[d].cpu().double()
        assert bool(torch.isfinite(torch.stack(got_h)).all()) and bool(torch.isfinite(got_c).all()), tag + ": not finite"
        for step in range(2):
            e = _cmp(f"{tag} dir {d} step {step}.h", got_h[step], refs[""][0][step], tols[step])
            fr = worst_fraction(got_h[step], refs[""][0][step], tols[step])
            out["h"] = max(out.get("h", (0.0, 0.0)), (e, fr))
        e = _cmp(f"{tag} dir {d}.c", got_c, refs[""][1], dc)
        out["c"] = max(out.get("c", (0.0, 0.0)), (e, worst_fraction(got_c, refs[""][1], dc)))
        r0 = kind == 0                    # the N(0,1) rows: every gate matters there
        if bool(r0.any()):
            for variant, (hs, _) in refs.items():
                if variant:
                    far(tag + f" dir {d}" + variant, got_h[1][r0], hs[1][r0], tols[1][r0])
    return out


GATE_ARGS = (0.0, 1e-4, -1e-4, 1e-3, -1e-3, 0.5, -0.5, 5.0, -5.0, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0, 1e4, -1e4)
GATE_SCALES = (1e-4, 1e-2, 1.0, 10.0)


def check_lstm_gate_functions(impl, name):
    """One step with W_hh = 0: the pre-activation is gates_x exactly, and saturated neighbours isolate one non-linearity in c':
        tanh     i = +1e4, f = -1e4:           c' = 1 tanh(x) + 0 c
        sigmoid  g = +1e4, f = -1e4, i = x:    c' = sigmoid(x) 1
        sigmoid  i = -1e4, c = 1, f = x:       c' = sigmoid(x) 1 + 0
    (sigmoid(+-1e4) and tanh(1e4) are exactly 1 / 0 / 1 in both forms), with o = +1e4 so that h' = tanh(c').  x: N(0,1) x {1e-4, 1e-2, 1, 10} by row,
    and GATE_ARGS in row 0.  c' is held to the ABSOLUTE per-gate bound NL_TANH / NL_SIGMOID alone; h' to (1 - tanh^2) of it plus NL_TANH.
    -> {"tanh": err, "sigmoid": err}"""
    dev, dtype = dev_of(impl), LSTM_DTYPES[name]
    b, hid = 16, 64
    g = gen(9)
    x = torch.randn(b, hid, generator=g) * torch.tensor(GATE_SCALES).repeat(b // 4).view(b, 1)
    x[0, :len(GATE_ARGS)] = torch.tensor(GATE_ARGS)
    big = torch.full((b, hid), 1e4)
    zero = torch.zeros(4 * hid, hid)
    wp, idx = product_regroup([zero, zero])
    wm, ws = pack_w(name, wp[0], dev)
    out = {}
    xd = x.double()
    for what, (gi, gf, gg), c0, want, nl in (("tanh", (big, -big, x), 0.7, torch.tanh(xd), NL_TANH[name]),
                                             ("sigmoid", (x, -big, big), 0.7, torch.sigmoid(xd), NL_SIGMOID[name]),
                                             ("sigmoid", (-big, x, torch.zeros(b, hid)), 1.0, torch.sigmoid(xd), NL_SIGMOID[name])):
        gates = torch.cat([gi, gf, gg, big], -1)                          # torch layout [i | f | g | o]
        gx = to_product_gates(torch.stack([gates, gates]), idx)[:, :4 * hid].contiguous().to(dev)
        c, hout = torch.full((b, hid), c0, device=dev), nans(dev, b, hid)
        impl.lstm_step(dtype, torch.tanh(torch.randn(b, hid, generator=g)).to(dev), wm, gx, c, hout, w_scale=ws)
        tag = f"lstm gate functions[{name} {what} of {'f' if c0 == 1.0 else 'g' if what == 'tanh' else 'i'}]"
        out[what] = max(out.get(what, 0.0), _cmp(tag + ".c", c, want, nl))
        tc = torch.tanh(want)
        _cmp(tag + ".h", hout, tc, (1 - tc ** 2) * nl + NL_TANH[name] + EPS32)
    return out


LAYER_CASES = [(hid, b, t) for hid in (256, 512) for (b, t) in ((1, 1), (3, 2), (17, 33), (65, 5))] + [(256, 3, 415)]
LAYER_FLOOR = 8 * EPS32
LAYER_IN = 32


def torch_lstm(w, x, dtype):
    """torch.nn.LSTM(bidirectional=True, batch_first=True) with weight_hh = w and the identity as input projection: input column block d feeds
    direction d unchanged (exact: products with 1 and sums with 0), so the recurrence sees exactly the gates it is given.  x (B, T, 8H)."""
    hid = w[0].shape[1]
    lstm = torch.nn.LSTM(8 * hid, hid, num_layers=1, bidirectional=True, batch_first=True).to(dtype)
    with torch.no_grad():
        for d, sfx in enumerate(("", "_reverse")):
            getattr(lstm, "weight_hh_l0" + sfx).copy_(w[d])
            wi = getattr(lstm, "weight_ih_l0" + sfx)
            wi.zero_()
            wi[:, 4 * hid * d:4 * hid * (d + 1)] = torch.eye(4 * hid, dtype=dtype)
            getattr(lstm, "bias_ih_l0" + sfx).zero_()
            getattr(lstm, "bias_hh_l0" + sfx).zero_()
        return lstm(x.to(dtype))[0]


def written_out_layer(w, gates, reverse=True, **kw):
    """The bidirectional layer from `cell64` in float64: gates (2, B, T, 4H) in torch's layout -> (B, T, 2H).  Wrong variants: the backward
    direction run forward in time (reverse = False), `carry = False` (the cell state reset at every step), and those of `cell64`."""
    carry = kw.pop("carry", True)
    _, b, t, n = gates.shape
    hid = n // 4
    out = torch.zeros(b, t, 2 * hid, dtype=torch.float64)
    for d in range(2):
        h, c = torch.zeros(b, hid, dtype=torch.float64), torch.zeros(b, hid, dtype=torch.float64)
        for s in (range(t - 1, -1, -1) if d == 1 and reverse else range(t)):
            h, c = cell64(gates[d][:, s].double(), h, c if carry else torch.zeros_like(c), w[d].double(), **kw)
            out[:, s, d * hid:(d + 1) * hid] = h
    return out


@functools.lru_cache(maxsize=None)
def layer_case(hid, b, t):
    """Seeded weights and gates of one layer, the float64 reference and the two fp32 restatements, computed once per case:
    gates = x W_ih^T + b_ih + b_hh in float64 from a 32-wide input, rounded to fp32 — the kernels AND the reference are given that fp32 value.
    -> dict(w, gates, ref (B, T, 2H) float64, err32 = the larger error of fake_ops.lstm_layer (the step arithmetic restated in fp32 torch) and
    torch.nn.LSTM in fp32 against ref)."""
    g = gen(10000 * hid + 100 * b + t)
    w = [torch.randn(4 * hid, hid, generator=g) / hid ** 0.5 for _ in range(2)]
    x = torch.randn(b, t, LAYER_IN, generator=g, dtype=torch.float64)
    gates = torch.stack([(x @ (torch.randn(4 * hid, LAYER_IN, generator=g, dtype=torch.float64) / LAYER_IN ** 0.5).t()
                          + 0.2 * torch.randn(4 * hid, generator=g, dtype=torch.float64)).float() for _ in range(2)])
    xin = torch.cat([gates[0], gates[1]], -1)
    ref = torch_lstm(w, xin, torch.float64)
    e_torch = float((torch_lstm(w, xin, torch.float32).double() - ref).abs().max())
    e_fake = float((run_layer(F, w, gates).double() - ref).abs().max())
    return dict(w=w, gates=gates, ref=ref, err32=max(e_torch, e_fake), err_torch=e_torch, err_fake=e_fake)


def run_layer(impl, w, gates):
    """`impl.lstm_layer` in split-f16 on the product-layout operands; gates_x and hseq are blocks of NaN (B, T + 1, . + 32) buffers."""
    dev = dev_of(impl)
    _, b, t, n = gates.shape
    hid = n // 4
    wp, idx = product_regroup(w)
    packed = [pack_w("f16x3", m, dev) for m in wp]
    gbuf, hbuf = nans(dev, b, t + 1, 8 * hid + 32), nans(dev, b, t + 1, 2 * hid + 32)
    gblk, hblk = (slice(None), slice(0, t), slice(16, 16 + 8 * hid)), (slice(None), slice(0, t), slice(16, 16 + 2 * hid))
    gbuf[gblk] = to_product_gates(gates, idx).to(dev)
    sync = impl.lstm_layer_sync(b, hid, dev)
    impl.lstm_layer(F16X3, gbuf[gblk], [p[0] for p in packed], [p[1] for p in packed], hbuf[hblk], sync)
    if dev == "cuda":
        torch.cuda.synchronize()
    impl.lstm_layer_check(sync)
    _nan_outside(f"lstm_layer[H={hid} B={b} T={t}]", hbuf, *hblk)
    return hbuf[hblk].cpu()


def check_lstm_layer(impl, hid, b, t):
    """The growth of the error over T steps has no useful closed form: the kernel may be 4 x as far from float64 as the fp32 restatements on the
    CPU are (a different but equally valid fp32 order), floor 8 EPS32.  -> (fp32-restatement error, error of `impl`)."""
    case = layer_case(hid, b, t)
    tag = f"lstm_layer[H={hid} B={b} T={t}]"
    got = run_layer(impl, case["w"], case["gates"])
    tol = max(4 * case["err32"], LAYER_FLOOR)
    print(f"{tag}: fp32 restatement err {case['err32']:.3e} (fake_ops {case['err_fake']:.3e}, torch.nn.LSTM fp32 {case['err_torch']:.3e})")
    err = _cmp(tag, got, case["ref"], tol)
    if t <= 33:
        w, gates = case["w"], case["gates"]
        _cmp(tag + ": the written-out cell vs torch.nn.LSTM, both float64", written_out_layer(w, gates), case["ref"], 1e-12)
        far(tag + " vs gate order i, f, o, g", got, written_out_layer(w, gates, order="ifog"), tol)
        far(tag + " vs sigmoid on the cell gate", got, written_out_layer(w, gates, cell_sigmoid=True), tol)
        if t > 1:
            far(tag + " vs the backward direction not time-reversed", got, written_out_layer(w, gates, reverse=False), tol)
            far(tag + " vs the cell state not carried", got, written_out_layer(w, gates, carry=False), tol)
    return case["err32"], err


# ---------------------------------------------------------------------------------------------------------------------------------
# softmax2_mix: out = softmax(sel[:, :2]) . (c1, c2), one thread per entry
# ---------------------------------------------------------------------------------------------------------------------------------
MIX_GAPS = (0.0, 1e-3, -1e-3, 30.0, -30.0, 200.0, -200.0)
MIX_BASES = (0.0, -5.0, 100.0)         # base 100: exp() without the max subtraction overflows fp32
MIX_C = 130


def check_softmax2_mix(impl):
    """sel = (base, base + gap).  tol per entry: 5 u (|c1| + |c2|) + 2 u (w1 |c1| + w2 |c2|) + u |out| — each weight is within 5 u ABSOLUTE: the gap
    d = |a - b| carries u d into exp(-d), (d + 2) u relative with expf's ulp, which weighs e^-d / (1 + e^-d) (d e^-d <= 0.37), then 1 + e, the
    division(s): <= 5 u; the two products and the sum round once each."""
    dev = dev_of(impl)
    rows = [(base, base + gap) for base in MIX_BASES for gap in MIX_GAPS]
    m = len(rows)
    g = gen(21)
    sb, c1b, c2b = torch.randn(m, 5, generator=g), torch.randn(m + 1, MIX_C + 3, generator=g), torch.randn(m, MIX_C + 7, generator=g)
    sb[:, 1:3] = torch.tensor(rows)
    sel, c1, c2 = sb[:, 1:], c1b[1:, 3:], c2b[:, 2:2 + MIX_C]
    ob = nans(dev, m + 2, MIX_C + 6)
    blk = (slice(1, m + 1), slice(4, 4 + MIX_C))
    impl.softmax2_mix(sb.to(dev)[:, 1:], c1b.to(dev)[1:, 3:], c2b.to(dev)[:, 2:2 + MIX_C], ob[blk])
    _nan_outside("softmax2_mix", ob, *blk)
    wgt = torch.softmax(sel[:, :2].double(), 1)
    ref = wgt[:, :1] * c1.double() + wgt[:, 1:] * c2.double()
    tol = 5 * EPS32 * (c1.abs() + c2.abs()).double() + 2 * EPS32 * (wgt[:, :1] * c1.abs() + wgt[:, 1:] * c2.abs()) + EPS32 * ref.abs()
    err = _cmp("softmax2_mix", ob[blk], ref, tol)
    frac = worst_fraction(ob[blk].cpu().double(), ref, tol)
    big = (sel[:, 0] - sel[:, 1]).abs() >= 30
    far("softmax2_mix vs the weights swapped", ob[blk][big], (wgt[:, 1:] * c1.double() + wgt[:, :1] * c2.double())[big], tol[big])
    e = torch.exp(sel[:, :2])                                             # fp32 without the max subtraction: inf / inf at base 100
    far("softmax2_mix vs no max subtraction", ob[blk], (e[:, :1] / e.sum(1, keepdim=True)) * c1 + (e[:, 1:] / e.sum(1, keepdim=True)) * c2, tol)
    return err, frac
