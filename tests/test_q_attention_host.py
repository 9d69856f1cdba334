"""Host side of the fused cross-attention site (emage_q_attention), no GPU needed: when `_decoder_layer` takes the one launch and when it keeps
the two, that it hands the fused launch the operands the two launches get, and that the entry points refuse what they do not support."""
import types

import pytest
import torch

import common
import fake_ops
from pantomatrix_amd import _lib, ops
from pantomatrix_amd._lib import F16X3, H2

D, T, H = 768, 64, 4


def _as_cuda(monkeypatch, model, precision_h2=True, cus=256):
    """A launch context that looks like an EMAGE_H2 forward on a GPU of `cus` CUs (only `_fused_cross_attn` reads it)."""
    monkeypatch.setattr(torch.cuda, "get_device_properties", lambda dev: types.SimpleNamespace(multi_processor_count=cus))
    return types.SimpleNamespace(h2=precision_h2, h2dt=H2 if precision_h2 else F16X3, dev=types.SimpleNamespace(type="cuda"))


def test_predicate_keeps_the_two_launches_outside_the_fused_shape(monkeypatch):
    model, _ = common.product_models(precision="f16x3")
    model.eval()
    cx = _as_cuda(monkeypatch, model)
    fused = lambda b=64, t=T, tk=T, c=cx: model._fused_cross_attn(c, b, t, tk, D, H)
    assert model.fuse_cross_attention and fused()
    assert fused(b=400)                                    # no 16-clip floor and no small ceiling: the 64 x 64 tile carries ca.q at every such row count
    assert not fused(t=6, tk=6) and not fused(t=6) and not fused(tk=65)          # tail windows (the body memory of one has T + 1 frames)
    assert not fused(b=63)                                 # fewer (clip, head) workgroups than CUs
    assert not fused(b=407)                                # 26 048 rows: emage_gemm would leave the 64 x 64 tile (20 M rows x k on 256 CUs)
    assert not fused(c=_as_cuda(monkeypatch, model, precision_h2=False))         # fp32 / bf16 / F16X3 forwards
    assert not fused(c=types.SimpleNamespace(h2=True, h2dt=H2, dev=types.SimpleNamespace(type="cpu")))
    model.train()
    assert not fused()
    model.eval()
    model.fuse_cross_attention = False
    assert not fused()
    assert ops.q_attention_supported(H2, 64, 64, 768, 4) and ops.q_attention_supported(ops.h2_shifted(3), 64, 64, 768, 4)
    assert not ops.q_attention_supported(F16X3, 64, 64, 768, 4) and not ops.q_attention_supported(H2, 64, 65, 768, 4)
    assert not ops.q_attention_supported(H2, 64, 64, 512, 4) and not ops.q_attention_supported(H2, 64, 64, 768, 8)


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_decoder_layer_falls_back_and_fused_operands_match(monkeypatch, precision):
    """Through the CPU stand-ins: a forward never reaches `ops.q_attention` on its own (no GPU: the two launches); with the predicate forced
    on for the EMAGE_H2 forward, `_decoder_layer` hands the fused launch exactly the operands that reproduce the two launches' outputs."""
    model, _ = common.product_models(precision=precision)
    audio, spk, motion, mask = common.window_inputs(1)
    calls = []

    def q_attention(dtype, a, w, bias, k, vt, vt_rows, out, b, *, w_scale, a_scale=None, ln=None, ln_eps=1e-5):
        calls.append((tuple(a.shape), tuple(k.shape), vt_rows, ln is not None))
        q = torch.empty(b * T, D)
        fake_ops.gemm(dtype, a, w, bias, out_f32=q, n=D, cp=D, w_scale=w_scale, a_scale=a_scale, ln=ln, ln_eps=ln_eps)
        fake_ops.attention(dtype, q, k, vt, vt_rows, out, b, H, T, T, D // H)

    monkeypatch.setattr(ops, "q_attention", q_attention)
    with fake_ops.installed(), torch.no_grad():
        ref = model.forward(audio, spk, motion, mask)
        n_att = fake_ops.CALLS.count("attention")
        short = model.forward(audio[:, :6 * 533], spk, motion[:, :6], mask[:, :6])       # a tail-sized window
    assert not calls and n_att >= 15 and all(torch.isfinite(v).all() for v in short.values() if torch.is_tensor(v))
    if precision != "f16x3":
        return
    monkeypatch.setattr(type(model), "_fused_cross_attn", lambda self, cx, b, t, tk, d, h: cx.h2 and not self.training and t == tk == T)
    with fake_ops.installed(), torch.no_grad():
        got = model.forward(audio, spk, motion, mask)
        short2 = model.forward(audio[:, :6 * 533], spk, motion[:, :6], mask[:, :6])
    assert len(calls) == 15 and all(c[0] == (T, D) and c[1] == (T, D) for c in calls)
    assert sorted({c[2] for c in calls}) == [D, 4 * D, 8 * D]              # the refinement layers' own memory, the face stack's, the body stack's
    for k, v in ref.items():
        if torch.is_tensor(v):
            assert torch.equal(v, got[k]), k
            assert torch.equal(short[k], short2[k]), k


def test_entry_points_refuse_before_any_launch():
    lib = _lib.load()
    arr = (_lib.QAttentionProblem * 5)()
    assert lib.emage_q_attention(H2, None, T, T, D, H, None) == -1
    assert lib.emage_q_attention(H2, arr, T, T, D, H, None) == -1                    # null pointers
    assert lib.emage_q_attention_grouped(H2, arr, 0, T, T, D, H, None) == -1
    assert lib.emage_q_attention_grouped(H2, arr, 5, T, T, D, H, None) == -1
    arr[0].A = arr[0].W = arr[0].bias = arr[0].k = arr[0].vt = arr[0].out = 4096     # aligned, never dereferenced: every call below is refused
    arr[0].lda = arr[0].ldo = arr[0].ldk = arr[0].vt_rows = D
    arr[0].ldvt, arr[0].B, arr[0].a_scale, arr[0].w_scale = T, 1, 16.0, 1.0
    assert lib.emage_q_attention(H2, arr, T, 32, D, H, None) == -1 and lib.emage_q_attention(F16X3, arr, T, T, D, H, None) == -1
    assert lib.emage_q_attention(H2, arr, 32, T, D, H, None) == -1 and lib.emage_q_attention(H2, arr, T, T, 512, H, None) == -1
    for field, bad in (("ldvt", 48), ("ldk", D + 2), ("lda", D + 4), ("ldo", D - 8), ("vt_rows", D - 1), ("A", 4100), ("k", 4104), ("B", 1 << 20)):
        keep = getattr(arr[0], field)
        setattr(arr[0], field, bad)
        assert lib.emage_q_attention(H2, arr, T, T, D, H, None) == -1, field
        setattr(arr[0], field, keep)
