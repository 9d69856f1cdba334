"""emage_q_attention (csrc/q_attention.hip): one cross-attention site in one launch.  Its `att` image must be bit for bit what the two-launch
sequence it replaces writes — the q projection (emage_gemm: q float32) followed by emage_attention on the layer's memory K / V^T — for plain
and LayerNorm-folded operands, with and without an activation shift, single and grouped; unsupported arguments are refused before any
launch; and the model's outputs must not move when the fused path is switched on."""
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
LAYERS = 2                  # K / V^T are layer 1 of a 2-layer memory: a wrong pitch or row offset cannot pass


def _g(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def _site(b, fold, shift, seed):
    """Operands of one site on the device, built once per case and never written again:
    (dtype, A image, packed W, bias, w_scale, ln or None, k view, V^T view, vt_rows)."""
    from pantomatrix_amd.modeling_emage_audio import _Packed
    dt = ops.h2_shifted(shift)
    sc = ops.act_scale(dt)
    g = _g(seed)
    m = b * T
    x = torch.randn(m, D, generator=g) * 1.5 + 0.3
    wq, bq = torch.randn(D, D, generator=g) / math.sqrt(D), torch.randn(D, generator=g) * 0.1
    kbuf = (torch.randn(m, LAYERS * D, generator=g) * 1.2).to(DEV)
    vtbuf = torch.randn(b, LAYERS * D, T, generator=g).to(DEV)
    mem = (kbuf[:, D:], vtbuf[:, D:], LAYERS * D)           # pointer offsets 768 and 768 Tp, ldk = vt_rows = 2 x 768
    if not fold:
        w_p, w_s = ops.split_f16_weights_h2(wq.to(DEV))
        return (dt, ops.h2_pack(x, sc).to(DEV), w_p, bq.to(DEV), w_s, None, *mem)
    # folded LayerNorm: A is the raw pre-norm sum s = x + a W_o^T + b_o, its row statistics written by a real producer launch (st_out)
    a = torch.randn(m, D, generator=g)
    wo, bo = torch.randn(D, D, generator=g) / math.sqrt(D), torch.randn(D, generator=g) * 0.1
    gamma, beta = 1.0 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    wo_p, wo_s = ops.split_f16_weights_h2(wo.to(DEV))
    s_img, st = torch.zeros(m, D, device=DEV), torch.zeros(m, D // 32, 2, device=DEV)
    ops.gemm(dt, ops.h2_pack(a, sc).to(DEV), wo_p, bo.to(DEV), None, ops.h2_pack(x, sc).to(DEV), s_img, None, None, n=D, cp=D, w_scale=wo_s,
             res_h2=True, stats_out=st)
    wf, bf, c = _Packed._fold_norm(type("P", (), {"p": {"n.weight": gamma, "n.bias": beta}})(), wq, bq, "n")
    w_p, w_s = ops.split_f16_weights_h2(wf.to(DEV))
    return (dt, s_img, w_p, bf.to(DEV).contiguous(), w_s, (st, c.to(DEV).contiguous()), *mem)


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _two_launches(dt, a, w, bias, w_s, ln, k, vt, vt_rows, b):
    q = _nan(b * T, D)
    ops.gemm(dt, a, w, bias, None, None, None, q, None, n=D, cp=D, w_scale=w_s, ln=ln)
    att = _nan(b * T, D)
    ops.attention(dt, q, k, vt, vt_rows, att, b, H, T, T, D // H)
    return att


def _fused(dt, a, w, bias, w_s, ln, k, vt, vt_rows, b):
    att = _nan(b * T, D)
    ops.q_attention(dt, a, w, bias, k, vt, vt_rows, att, b, w_scale=w_s, ln=ln)
    return att


def _same_bits(x, y):
    return torch.equal(x.view(torch.int32), y.view(torch.int32))


# B = 1, 3, 17: 4, 12 and 68 workgroups (17 leaves a ragged last XCD run); the q projection takes the 64 x 64 tile at every one of them
@pytest.mark.parametrize("b,fold,shift", [(b, f, s) for b in (1, 3, 17) for f in (False, True) for s in (0, 3)])
def test_fused_site_is_bit_identical_to_projection_plus_attention(b, fold, shift):
    site = _site(b, fold, shift, 3000 + 10 * b + 2 * fold + shift)
    ref = _two_launches(*site, b)
    got = _fused(*site, b)
    torch.cuda.synchronize()
    assert torch.isfinite(ops.h2_unpack(ref, ops.act_scale(site[0]))).all()
    assert _same_bits(got, ref), f"max |diff| {float((ops.h2_unpack(got) - ops.h2_unpack(ref)).abs().max()):.3e}"


@pytest.mark.parametrize("n", [1, 2, 3])
def test_grouped_sites_in_lockstep(n):
    """Sites at the heads of lock-step chains share one grouped launch; each problem's bits are those of its own single launch."""
    cases = [(17, True), (3, False), (1, True)][:n]
    sites = [_site(b, fold, 0, 4000 + i) for i, (b, fold) in enumerate(cases)]
    bs = [b for b, _ in cases]
    refs = [_fused(*s, b) for s, b in zip(sites, bs)]
    outs = [_nan(b * T, D) for b in bs]
    with ops.lockstep() as ls:
        for (dt, a, w, bias, w_s, ln, k, vt, vt_rows), b, o in zip(sites, bs, outs):
            with ls.chain():
                ops.q_attention(dt, a, w, bias, k, vt, vt_rows, o, b, w_scale=w_s, ln=ln)
    torch.cuda.synchronize()
    assert ls.launches == ([("q_attention", 1)] if n == 1 else [("group", n)])
    for o, r in zip(outs, refs):
        assert _same_bits(o, r)


def test_refusals():
    """Misaligned pointers, Tk != 64, a dtype that is not EMAGE_H2 and ldvt = 48 are refused before any launch: the output keeps its NaNs."""
    b = 2
    dt, a, w, bias, w_s, _, k, vt, vt_rows = _site(b, False, 0, 11)
    out = _nan(b * T, D)
    lib = _lib.load()

    def call(dtype=H2, tk=T, **kw):
        f = dict(A=a.data_ptr(), W=w.data_ptr(), bias=bias.data_ptr(), ln_stats=None, ln_c=None, k=k.data_ptr(), vt=vt.data_ptr(), out=out.data_ptr(),
                 lda=D, ldk=LAYERS * D, ldvt=T, vt_rows=vt_rows, ldo=D, B=b, a_scale=16.0, w_scale=w_s, ln_eps=0.0)
        f.update(kw)
        pr = _lib.QAttentionProblem(**f)
        return lib.emage_q_attention(dtype, ctypes.byref(pr), T, tk, D, H, None)

    for name in ("A", "W", "bias", "k", "vt", "out"):
        assert call(**{name: dict(A=a, W=w, bias=bias, k=k, vt=vt, out=out)[name].data_ptr() + 4}) == -1, name
    assert call(tk=32) == -1 and call(tk=96) == -1
    assert call(dtype=F16X3) == -1 and call(dtype=0) == -1
    assert call(ldvt=48) == -1 and call(ldvt=32) == -1 and call(ldk=LAYERS * D + 2) == -1 and call(vt_rows=D - 1) == -1
    assert call(lda=D + 4) == -1 and call(ldo=D - 8) == -1 and call(B=0) == -1
    assert call(ln_stats=bias.data_ptr()) == -1 and call(ln_stats=bias.data_ptr(), ln_c=bias.data_ptr(), ln_eps=0.0) == -1
    assert lib.emage_q_attention(H2, None, T, T, D, H, None) == -1
    arr = (_lib.QAttentionProblem * 5)()
    assert lib.emage_q_attention_grouped(H2, arr, 0, T, T, D, H, None) == -1 and lib.emage_q_attention_grouped(H2, arr, 5, T, T, D, H, None) == -1
    # ... and through the op layer they raise
    with pytest.raises(ops.EmageKernelError):
        ops.q_attention(F16X3, a, w, bias, k, vt, vt_rows, out, b, w_scale=w_s)
    with pytest.raises(ops.EmageKernelError):
        ops.q_attention(dt, a, w, bias, k, torch.zeros(b, LAYERS * D, 48, device=DEV), vt_rows, out, b, w_scale=w_s)
    with pytest.raises(ops.EmageKernelError):
        ops.q_attention(dt, torch.zeros(b * T * D + 1, device=DEV)[1:].view(b * T, D), w, bias, k, vt, vt_rows, out, b, w_scale=w_s)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    assert call() == 0                    # the accepted call, last: everything above left the device untouched
    torch.cuda.synchronize()
    assert torch.isfinite(ops.h2_unpack(out)).all()


class _Count:
    """ops._TRACE hook: the recorded calls behind every launch, by op name."""

    def __init__(self):
        self.n = {}

    def tag(self):
        return None

    def fire(self, kind, entries, launch):
        for e in entries:
            self.n[e[0]] = self.n.get(e[0], 0) + 1
        return launch()


@pytest.mark.parametrize("frames", [128, 70])
def test_model_outputs_unchanged(frames):
    """EmageAudioModel.inference on 64 clips (the flagship batch; 70 frames: the 6-frame tail window takes the two-launch form): every
    cross-attention site of a full window goes through the fused launch, and every output is bit-identical with the fused sites on and off,
    eager and under ClipRunner's graph replay."""
    from tools import workloads as common
    from pantomatrix_amd import synthetic
    from pantomatrix_amd import modeling_emage_audio as M
    from pantomatrix_amd.runtime import ClipRunner
    b = 64
    n = synthetic.samples_for_frames(frames)
    audio = synthetic.synthetic_audio(b, n).to(DEV)
    model, vq = common.product_models(precision="f16x3", device=DEV)
    spk = torch.zeros(b, 1, dtype=torch.long, device=DEV)
    sites = M.spec.N_CROSS_LAYERS + M.spec.N_FACE_LAYERS + 3            # per window: both decoder stacks and the three refinement layers
    results = {}
    for fuse in (True, False):
        model.fuse_cross_attention = fuse
        counts = _Count()
        ops._TRACE[0] = counts
        try:
            with torch.no_grad():
                eager = model.inference(audio, spk, vq)
        finally:
            ops._TRACE[0] = None
        assert counts.n.get("q_attention", 0) == (sites * (frames // T) if fuse else 0), counts.n
        r = ClipRunner(model, vq, b, n, use_graph=True)
        replay = r(audio)
        torch.cuda.synchronize()
        results[fuse] = (eager, replay)
    (e1, r1), (e0, r0) = results[True], results[False]
    keys = [k for k in e1 if torch.is_tensor(e1[k])]
    assert keys and all(torch.equal(e1[k], e0[k]) for k in keys), [k for k in keys if not torch.equal(e1[k], e0[k])]
    assert len(r1) == 3 and all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(r1, r0))
