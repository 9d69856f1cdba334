"""emage_qm_attention (csrc/q_attention.hip): a decoder stack's cross-attention site that computes its memory K / V^T itself from the memory
feature image and the stack's composed k|v operand.  Its `att` image must be bit for bit what the composed two-launch form writes — emage_gemm
(K float32, V^T float32 of every layer) followed by emage_q_attention on this layer's slice — for both feature widths, plain and
LayerNorm-folded q operands, with and without an activation shift, single and grouped, with the features a row window of a longer tensor and
the layer a non-zero slice of the stacked operand.  Independently it is held against float64 torch of the UNCOMPOSED chain (memory projection,
then K / V projection, then attention): the composed operand is one more rounding site than the parent's three launches have, so the new form
may be up to twice as far from float64 as the parent's form is on the same inputs.

Measured on MI355X over the 24 cases below (max |att - float64| over a case's outputs; att is O(1)):
    parent's uncomposed form  0.98e-06 .. 3.40e-06 (largest: b = 17, km = 256, no fold, shift 3)
    emage_qm_attention        0.69e-06 .. 3.49e-06 (the same case; largest ratio to the parent's on one case: 1.16)
"""
import ctypes
import functools
import math

import pytest
import torch

from pantomatrix_amd import _lib, ops
from pantomatrix_amd._lib import F16X3, H2

pytestmark = pytest.mark.gpu
DEV = "cuda"
D, T, H = 768, 64, 4
LAYERS, LAYER = 3, 1        # the site is layer 1 of a 3-layer stack: a wrong row offset into the stacked operand cannot pass
PAD_ROWS = T                # the features are rows [T, T + B T) of a longer tensor (the hoisted layout: one window of several)


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _dummy(params):
    return type("P", (), {"p": params})()


@functools.lru_cache(maxsize=None)
def _site(b, km, fold, shift, seed, layer=LAYER):
    """Operands of one site on the device and the float32 parameters behind them, built once per case and never written again."""
    from pantomatrix_amd.modeling_emage_audio import _Packed
    dt = ops.h2_shifted(shift)
    sc = ops.act_scale(dt)
    g = _g(seed)
    m = b * T
    x = torch.randn(m, D, generator=g) * 1.5 + 0.3
    wq, bq = torch.randn(D, D, generator=g) / math.sqrt(D), torch.randn(D, generator=g) * 0.1
    feat = torch.randn(m + 2 * PAD_ROWS, km + 8, generator=g)                     # pitch km + 8: a wrong pitch cannot pass either
    wp, bp = torch.randn(D, km, generator=g) / math.sqrt(km), torch.randn(D, generator=g) * 0.1
    wkv, bkv = torch.randn(2 * LAYERS * D, D, generator=g) / math.sqrt(D), torch.randn(2 * LAYERS * D, generator=g) * 0.1
    feat_img = ops.h2_pack(feat, sc).to(DEV)
    mem = feat_img[PAD_ROWS:PAD_ROWS + m]
    wc, bc = _Packed._compose(_dummy({"p.weight": wp, "p.bias": bp}), wkv, bkv, "p")
    wc_p, wc_s = ops.split_f16_weights_h2(wc.to(DEV))
    plain = dict(wp=ops.split_f16_weights_h2(wp.to(DEV)), bp=bp.to(DEV), wkv=ops.split_f16_weights_h2(wkv.to(DEV)), bkv=bkv.to(DEV))
    f64 = dict(feat=ops.h2_unpack(mem[:, :km].contiguous(), sc).double().cpu(), wp=wp.double(), bp=bp.double(), wq=wq.double(), bq=bq.double(),
               wk=wkv[layer * D:(layer + 1) * D].double(), bk=bkv[layer * D:(layer + 1) * D].double(),
               wv=wkv[(LAYERS + layer) * D:(LAYERS + layer + 1) * D].double(), bv=bkv[(LAYERS + layer) * D:(LAYERS + layer + 1) * D].double())
    kv = (mem, km, wc_p, bc.to(DEV), wc_s, layer)
    if not fold:
        w_p, w_s = ops.split_f16_weights_h2(wq.to(DEV))
        a = ops.h2_pack(x, sc).to(DEV)
        f64["x"] = ops.h2_unpack(a, sc).double().cpu()
        return (dt, a, w_p, bq.to(DEV), w_s, None, kv, plain, f64)
    # folded LayerNorm: A is the raw pre-norm sum s = x + a W_o^T + b_o, its row statistics written by a real producer launch (st_out)
    a = torch.randn(m, D, generator=g)
    wo, bo = torch.randn(D, D, generator=g) / math.sqrt(D), torch.randn(D, generator=g) * 0.1
    gamma, beta = 1.0 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    wo_p, wo_s = ops.split_f16_weights_h2(wo.to(DEV))
    s_img, st = torch.zeros(m, D, device=DEV), torch.zeros(m, D // 32, 2, device=DEV)
    ops.gemm(dt, ops.h2_pack(a, sc).to(DEV), wo_p, bo.to(DEV), None, ops.h2_pack(x, sc).to(DEV), s_img, None, None, n=D, cp=D, w_scale=wo_s,
             res_h2=True, stats_out=st)
    wf, bf, c = _Packed._fold_norm(_dummy({"n.weight": gamma, "n.bias": beta}), wq, bq, "n")
    w_p, w_s = ops.split_f16_weights_h2(wf.to(DEV))
    s = ops.h2_unpack(s_img, sc).double().cpu()
    f64["x"] = torch.nn.functional.layer_norm(s, (D,), gamma.double(), beta.double(), 1e-5)
    return (dt, s_img, w_p, bf.to(DEV).contiguous(), w_s, (st, c.to(DEV).contiguous()), kv, plain, f64)


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _kv_launch(dt, mem, w_p, bias, w_s, cp, b):
    """emage_gemm as `_memory_kv` issues it: K float32 (B T, LAYERS d) and V^T float32 (B, LAYERS d, T) of every layer."""
    k, vt = _nan(b * T, LAYERS * D), _nan(b, LAYERS * D, T)
    ops.gemm(dt, mem, w_p, bias, None, None, None, k, vt, n=2 * LAYERS * D, cp=cp, t_col0=LAYERS * D, t_rows=T, w_scale=w_s)
    return k, vt


def _q_site(dt, a, w, bias, w_s, ln, k, vt, layer, b):
    att = _nan(b * T, D)
    ops.q_attention(dt, a, w, bias, k[:, layer * D:(layer + 1) * D], vt[:, layer * D:], LAYERS * D, att, b, w_scale=w_s, ln=ln)
    return att


def _composed_two_launches(site, b):
    dt, a, w, bias, w_s, ln, (mem, km, wc_p, bc, wc_s, layer), _plain, _f64 = site
    k, vt = _kv_launch(dt, mem, wc_p, bc, wc_s, km, b)
    return _q_site(dt, a, w, bias, w_s, ln, k, vt, layer, b)


def _parent_three_launches(site, b):
    """The uncomposed form: the memory projection (an EMAGE_H2 image), the plain K / V launch on it, the fused q site."""
    dt, a, w, bias, w_s, ln, (mem, km, _wc, _bc, _ws, layer), plain, _f64 = site
    proj = _nan(b * T, D)
    ops.gemm(dt, mem, plain["wp"][0], plain["bp"], None, None, proj, None, None, n=D, cp=km, w_scale=plain["wp"][1])
    k, vt = _kv_launch(dt, proj, plain["wkv"][0], plain["bkv"], plain["wkv"][1], D, b)
    return _q_site(dt, a, w, bias, w_s, ln, k, vt, layer, b)


def _fused(site, b, out=None):
    dt, a, w, bias, w_s, ln, (mem, _km, wc_p, bc, wc_s, layer), _plain, _f64 = site
    att = _nan(b * T, D) if out is None else out
    ops.qm_attention(dt, a, w, bias, mem, wc_p, bc, LAYERS, layer, att, b, w_scale=w_s, wkv_scale=wc_s, ln=ln)
    return att


def _float64(site, b):
    f = site[-1]
    memory = f["feat"] @ f["wp"].T + f["bp"]
    q = (f["x"] @ f["wq"].T + f["bq"]).view(b, T, H, D // H).transpose(1, 2)
    k = (memory @ f["wk"].T + f["bk"]).view(b, T, H, D // H).transpose(1, 2)
    v = (memory @ f["wv"].T + f["bv"]).view(b, T, H, D // H).transpose(1, 2)
    p = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(D // H), dim=-1)
    return (p @ v).transpose(1, 2).reshape(b * T, D)


def _same_bits(x, y):
    return torch.equal(x.view(torch.int32), y.view(torch.int32))


# B = 1, 3, 17: 4, 12 and 68 workgroups (17 leaves a ragged last XCD run); 256 / 512 feature columns: 8 / 16 K-tiles on the ring of 2
@pytest.mark.parametrize("b,km,fold,shift", [(b, km, f, s) for b in (1, 3, 17) for km in (256, 512) for f in (False, True) for s in (0, 3)])
def test_site_is_bit_identical_to_composed_kv_launch_plus_q_site(b, km, fold, shift):
    site = _site(b, km, fold, shift, 7000 + 100 * b + km // 8 + 2 * fold + shift)
    sc = ops.act_scale(site[0])
    ref = _composed_two_launches(site, b)
    got = _fused(site, b)
    parent = _parent_three_launches(site, b)
    torch.cuda.synchronize()
    assert torch.isfinite(ops.h2_unpack(ref, sc)).all()
    assert _same_bits(got, ref), f"max |diff| {float((ops.h2_unpack(got, sc) - ops.h2_unpack(ref, sc)).abs().max()):.3e}"
    # ... and against float64 of the uncomposed chain: at most twice the parent's own distance (one rounding site more: the composed operand)
    want = _float64(site, b)
    err_parent = float((ops.h2_unpack(parent, sc).double().cpu() - want).abs().max())
    err_new = float((ops.h2_unpack(got, sc).double().cpu() - want).abs().max())
    print(f"b={b} km={km} fold={fold} shift={shift}: max|err| vs float64: parent's form {err_parent:.3e}, qm_attention {err_new:.3e}")
    assert err_parent > 0 and err_new <= 2 * err_parent, (err_new, err_parent)


def test_first_layer_of_the_stack():
    """Layer 0 (no row offset into the stacked operand) next to the layer-1 cases above."""
    site = _site(3, 256, True, 0, 7777, layer=0)
    ref, got = _composed_two_launches(site, 3), _fused(site, 3)
    torch.cuda.synchronize()
    assert _same_bits(got, ref)


@pytest.mark.parametrize("n", [1, 2])
def test_grouped_sites_in_lockstep(n):
    """Sites at the heads of lock-step chains (the face and the body stack) share one grouped launch; each problem's bits are its own launch's."""
    cases = [(3, 512, True), (17, 256, False)][:n]
    sites = [_site(b, km, fold, 0, 8000 + i) for i, (b, km, fold) in enumerate(cases)]
    bs = [c[0] for c in cases]
    refs = [_fused(s, b) for s, b in zip(sites, bs)]
    outs = [_nan(b * T, D) for b in bs]
    with ops.lockstep() as ls:
        for s, b, o in zip(sites, bs, outs):
            with ls.chain():
                _fused(s, b, out=o)
    torch.cuda.synchronize()
    assert ls.launches == ([("q_attention", 1)] if n == 1 else [("group", n)])        # logged with its family, the cross-attention sites
    for o, r in zip(outs, refs):
        assert _same_bits(o, r)


def test_refusals():
    """Misaligned pointers, unsupported shapes, a feature width that is no whole K-tile and a layer outside the stack are refused before any
    launch: the output keeps its NaNs."""
    b = 2
    dt, a, w, bias, w_s, _, (mem, km, wc_p, bc, wc_s, layer), _plain, _f64 = _site(b, 256, False, 0, 11)
    out = _nan(b * T, D)
    lib = _lib.load()
    ptrs = dict(A=a, W=w, bias=bias, mem=mem, Wkv=wc_p, bias_kv=bc, out=out)

    def call(dtype=H2, tk=T, **kw):
        f = dict(ln_stats=None, ln_c=None, lda=D, ldm=mem.stride(0), km=km, kv_layers=LAYERS, kv_layer=layer, ldo=D, B=b, a_scale=16.0,
                 w_scale=w_s, wkv_scale=wc_s, ln_eps=0.0, **{k: v.data_ptr() for k, v in ptrs.items()})
        f.update(kw)
        pr = _lib.QmAttentionProblem(**f)
        return lib.emage_qm_attention(dtype, ctypes.byref(pr), T, tk, D, H, None)

    for name, t in ptrs.items():
        assert call(**{name: t.data_ptr() + 4}) == -1, name
        assert call(**{name: None}) == -1, name
    assert call(tk=32) == -1 and call(dtype=F16X3) == -1 and call(dtype=0) == -1
    assert call(km=0) == -1 and call(km=48) == -1 and call(km=D + 32) == -1 and call(ldm=km - 8) == -1 and call(ldm=km + 4) == -1
    assert call(kv_layers=0) == -1 and call(kv_layer=LAYERS) == -1 and call(kv_layer=-1) == -1 and call(wkv_scale=0.0) == -1
    assert call(lda=D + 4) == -1 and call(ldo=D - 8) == -1 and call(B=0) == -1 and call(w_scale=-1.0) == -1
    assert call(ln_stats=bias.data_ptr()) == -1
    assert lib.emage_qm_attention(H2, None, T, T, D, H, None) == -1
    arr = (_lib.QmAttentionProblem * 5)()
    assert lib.emage_qm_attention_grouped(H2, arr, 0, T, T, D, H, None) == -1 and lib.emage_qm_attention_grouped(H2, arr, 5, T, T, D, H, None) == -1
    with pytest.raises(ops.EmageKernelError):
        ops.qm_attention(F16X3, a, w, bias, mem, wc_p, bc, LAYERS, layer, out, b, w_scale=w_s, wkv_scale=wc_s)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    assert call() == 0                    # the accepted call, last: everything above left the device untouched
    torch.cuda.synchronize()
    assert torch.isfinite(ops.h2_unpack(out)).all()


class _Count:
    """ops._TRACE hook: the recorded calls behind every launch, by operator (`qm_attention` calls carry the name of their family,
    `q_attention`, and their own in meta["op"])."""

    def __init__(self):
        self.n, self.family = {}, {}

    def tag(self):
        return None

    def fire(self, kind, entries, launch):
        for e in entries:
            name = e[3].get("op", e[0])
            self.n[name] = self.n.get(name, 0) + 1
            self.family[e[0]] = self.family.get(e[0], 0) + 1
        return launch()


@pytest.mark.parametrize("frames", [128, 70])
def test_model_outputs_unchanged(frames):
    """EmageAudioModel.inference on 64 clips (the flagship batch; 70 frames: the 6-frame tail window keeps the composed K / V launch and the
    two-launch sites): every stack site of a full window computes its own K / V^T, and every output is bit-identical with those sites on and
    off (off: one composed K / V launch per stack + the q sites), eager and under ClipRunner's graph replay."""
    from tools import workloads as common
    from pantomatrix_amd import synthetic
    from pantomatrix_amd import modeling_emage_audio as M
    from pantomatrix_amd.runtime import ClipRunner
    b = 64
    n = synthetic.samples_for_frames(frames)
    audio = synthetic.synthetic_audio(b, n).to(DEV)
    model, vq = common.product_models(precision="f16x3", device=DEV)
    assert model.compose_memory and model.fuse_memory_kv
    spk = torch.zeros(b, 1, dtype=torch.long, device=DEV)
    stack = M.spec.N_CROSS_LAYERS + M.spec.N_FACE_LAYERS
    results = {}
    for fuse in (True, False):
        model.fuse_memory_kv = fuse
        counts = _Count()
        ops._TRACE[0] = counts
        try:
            with torch.no_grad():
                eager = model.inference(audio, spk, vq)
        finally:
            ops._TRACE[0] = None
        full = frames // T
        assert counts.n.get("qm_attention", 0) == (stack * full if fuse else 0), counts.n
        assert counts.n.get("q_attention", 0) == (3 * full if fuse else (stack + 3) * full), counts.n
        assert counts.family.get("q_attention", 0) == (stack + 3) * full and "qm_attention" not in counts.family, counts.family
        r = ClipRunner(model, vq, b, n, use_graph=True)
        replay = r(audio)
        torch.cuda.synchronize()
        results[fuse] = (eager, replay)
    (e1, r1), (e0, r0) = results[True], results[False]
    keys = [k for k in e1 if torch.is_tensor(e1[k])]
    assert keys and all(torch.equal(e1[k], e0[k]) for k in keys), [k for k in keys if not torch.equal(e1[k], e0[k])]
    assert len(r1) == 3 and all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(r1, r0))
