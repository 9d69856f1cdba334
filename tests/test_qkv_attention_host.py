"""Host side of the fused self-attention site (emage_qkv_attention), no GPU needed: the entry points refuse every unsupported argument before
any launch, the lock-step walk groups the sites at the heads of its chains by kind, and the model's dispatch keeps the two-launch form
off the GPU and for shapes the kernel is not built for."""
import types

from pantomatrix_amd import _lib, ops
from pantomatrix_amd._lib import H2, F16X3

D, T, H = 768, 64, 4


def _call(**kw):
    # 16-byte aligned fake addresses: refused arguments never reach a launch
    ok = dict(A=1 << 20, lda=D, W=2 << 20, bias=3 << 20, ln_stats=None, ln_c=None, ln_eps=0.0, out=4 << 20, ldo=D, B=64, T=T, d=D, H=H,
              a_scale=16.0, w_scale=1024.0)
    dtype = kw.pop("dtype", H2)
    a = dict(ok, **kw)
    return _lib.load().emage_qkv_attention(dtype, *(a[k] for k in ok), None)


def test_unsupported_arguments_are_refused():
    for bad in (dict(dtype=F16X3), dict(dtype=0), dict(dtype=H2 | (13 << 8)), dict(T=32), dict(T=128), dict(d=512), dict(H=8),
                dict(A=None), dict(W=None), dict(bias=None), dict(out=None), dict(A=(1 << 20) + 4), dict(out=(4 << 20) + 8),
                dict(lda=D + 4), dict(lda=512), dict(ldo=D - 8), dict(B=0), dict(a_scale=0.0), dict(w_scale=-1.0),
                dict(ln_stats=5 << 20), dict(ln_stats=5 << 20, ln_c=6 << 20), dict(ln_stats=(5 << 20) + 4, ln_c=6 << 20, ln_eps=1e-5)):
        assert _call(**bad) == -1, bad


def test_grouped_entry_refuses_bad_counts():
    lib = _lib.load()
    arr = (_lib.QkvAttentionProblem * 5)()
    assert lib.emage_qkv_attention_grouped(H2, arr, 0, T, D, H, None) == -1
    assert lib.emage_qkv_attention_grouped(H2, arr, 5, T, D, H, None) == -1
    assert lib.emage_qkv_attention_grouped(H2, arr, 1, T, D, H, None) == -1          # null pointers


def test_supported_shapes():
    assert ops.qkv_attention_supported(H2, 64, 768, 4) and ops.qkv_attention_supported(ops.h2_shifted(3), 64, 768, 4)
    assert not ops.qkv_attention_supported(F16X3, 64, 768, 4)
    assert not ops.qkv_attention_supported(H2, 6, 768, 4) and not ops.qkv_attention_supported(H2, 64, 512, 4)


def test_lockstep_groups_heads_by_kind():
    """Heads of different kinds at one lock-step round go out as one grouped call per kind, in the order of their first head."""
    issued = []
    ls = ops.Lockstep(True)
    ls._issue = lambda e: issued.append(("one", e[0]))
    ls._issue_group = lambda es: issued.append(("group", es[0][0], len(es)))
    entry = lambda kind: (kind, None, (H2,), {})
    ls.chains = [[entry("qkv_attention"), entry("gemm")], [entry("gemm"), entry("gemm")], [entry("qkv_attention"), entry("gemm")]]
    ls.run()
    assert issued == [("group", "qkv_attention", 2), ("one", "gemm"), ("group", "gemm", 3)]


def test_model_dispatch_keeps_two_launches_off_the_gpu():
    from pantomatrix_amd.modeling_emage_audio import EmageAudioModel
    m = types.SimpleNamespace(fuse_self_attention=True, training=False)
    cx = types.SimpleNamespace(h2=True, h2dt=H2, dev=types.SimpleNamespace(type="cpu"))
    f = EmageAudioModel._fused_self_attn
    assert not f(m, cx, 64, 64, D, H)                                  # CPU: the fake ops restate only the two launches
    cx.dev.type = "cuda"
    for b, t, d, h, h2, train, on in ((64, 6, D, H, True, False, True), (64, 64, D, H, False, False, True), (64, 64, D, H, True, True, True),
                                       (64, 64, D, H, True, False, False), (8, 64, D, H, True, False, True)):
        cx.h2, m.training, m.fuse_self_attention = h2, train, on
        assert not f(m, cx, b, t, d, h), (b, t, h2, train, on)
