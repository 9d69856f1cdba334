"""Host side of `compose_memory` and of the stack sites that compute their own K / V^T (emage_qm_attention), no GPU needed: the composed
operands against the float64 two-step product, where they sit in the packing order, when the forward contracts the feature images and when a
site takes the new launch, what it hands that launch, and what the entry points refuse."""
import types

import numpy as np
import torch

import common
import fake_ops
import fake_qm_ops
from pantomatrix_amd import _lib, ops
from pantomatrix_amd import modeling_emage_audio as M
from pantomatrix_amd._lib import F16X3, H2

D, T, H = 768, 64, 4


def test_composed_operands_equal_the_float64_two_step_product():
    g = torch.Generator().manual_seed(5)
    kin, layers = 96, 2
    wp, bp = torch.randn(D, kin, generator=g) / kin ** 0.5, torch.randn(D, generator=g)
    wkv, bkv = torch.randn(2 * layers * D, D, generator=g) / D ** 0.5, torch.randn(2 * layers * D, generator=g)
    pk = type("P", (), {"p": {"proj.weight": wp, "proj.bias": bp}})()
    wc, bc = M._Packed._compose(pk, wkv, bkv, "proj")
    assert wc.dtype == bc.dtype == torch.float32 and wc.shape == (2 * layers * D, kin) and wc.is_contiguous()
    w64, b64 = wkv.double() @ wp.double(), wkv.double() @ bp.double() + bkv.double()
    # rounded ONCE: each element is the float32 nearest to the float64 product (half an ulp)
    assert bool(((wc.double() - w64).abs() <= 2.0 ** -24 * w64.abs() + 1e-45).all()) and bool(((bc.double() - b64).abs() <= 2.0 ** -24 * b64.abs() + 1e-45).all())
    a = torch.randn(32, kin, generator=g).double()
    two_step = (a @ wp.double().T + bp.double()) @ wkv.double().T + bkv.double()
    assert float((a @ wc.double().T + bc.double() - two_step).abs().max()) < 1e-5


def test_packing_builds_them_behind_the_plain_entries_and_follows_the_switch():
    model, _ = common.product_models(precision="f16x3")
    assert model.compose_memory and model.fuse_memory_kv
    c = model.config
    with fake_ops.installed(), torch.no_grad():
        on = model._engine()
        assert on.compose and on is model._engine()
        model.compose_memory = False
        off = model._engine()                                   # the switch is part of the staleness check: a new set
        assert off is not on and not off.compose
        train = model._engine(h2=False, train_only=True)
        model.compose_memory = True
        assert not train.compose and M._BODY_KV not in train.w
        fp32, _ = common.product_models(precision="fp32")
        assert not fp32._engine().compose and M._BODY_KV not in fp32._engine().w
    assert set(on.w) - set(off.w) == {M._BODY_KV, M._FACE_KV}
    assert on._n_operands == off._n_operands + 2                # ... packed LAST: no plain entry's place in the order (the scale cache's key) moves
    assert all(on.w[k]["ws"] == off.w[k]["ws"] for k in off.w if isinstance(off.w[k], dict) and "ws" in off.w[k])
    for key, proj, plain, layers, kin in ((M._BODY_KV, "audio_body_motion_proj", "cross.kv_all", M.spec.N_CROSS_LAYERS, c.audio_f),
                                          (M._FACE_KV, "audio_face_motion_proj", "face.kv_all", M.spec.N_FACE_LAYERS, c.audio_f + c.motion_f)):
        e, p = on.w[key], on.w[plain]
        assert e["n"] == p["n"] == 2 * layers * D and e["cp"] == e["k_real"] == kin and key not in on.origin and plain in on.origin
        wkv = torch.cat([on.p[nm][sl] for nm, _b, sl in on.origin[plain]]).double()
        bkv = torch.cat([on.p[b][sl] for _w, b, sl in on.origin[plain]]).double()
        w64 = wkv @ on.p[proj + ".weight"].double()
        hi, lo = fake_ops.h2_planes(e["w"], kin)
        np.testing.assert_allclose(((hi + lo) / e["ws"]).double().numpy(), w64.numpy(), rtol=0, atol=2.0 ** -21 * float(w64.abs().max()))
        np.testing.assert_allclose(e["b"].double().numpy(), (wkv @ on.p[proj + ".bias"].double() + bkv).numpy(), rtol=0, atol=1e-6)


def test_forward_contracts_the_feature_images(golden_dir):
    """With the switch on a window runs two contractions fewer (the two memory projections) and its K / V launches contract 256 / 512 columns;
    the outputs stay at the golden and at the uncomposed form to fp32 rounding; fp32 forwards ignore the switch."""
    import os
    model, _ = common.product_models(precision="f16x3")
    g = np.load(os.path.join(golden_dir, "forward_b1.npz"))
    audio, spk, motion, mask = common.window_inputs(1)
    outs, gemms = {}, {}
    with fake_ops.installed(), torch.no_grad():
        for compose in (True, False):
            model.compose_memory = compose
            fake_ops.CALLS.clear()
            outs[compose] = {k: v.clone() for k, v in model.forward(audio, spk, motion, mask).items() if torch.is_tensor(v)}
            gemms[compose] = fake_ops.CALLS.count("gemm")
    model.compose_memory = True
    assert gemms[True] == gemms[False] - 2, gemms
    for k, v in outs[True].items():
        np.testing.assert_allclose(v.numpy(), g[k], atol=3e-4, rtol=0)
        assert float((v - outs[False][k]).abs().max()) < 2e-5, k
    assert any(not torch.equal(v, outs[False][k]) for k, v in outs[True].items())          # a different association, not the same launches
    fp32, _ = common.product_models(precision="fp32")
    with fake_ops.installed(), torch.no_grad():
        n = {}
        for compose in (True, False):
            fp32.compose_memory = compose
            fake_ops.CALLS.clear()
            fp32.forward(audio, spk, motion, mask)
            n[compose] = fake_ops.CALLS.count("gemm")
    assert n[True] == n[False]


def _as_cuda(monkeypatch, cus=256, compose=True):
    monkeypatch.setattr(torch.cuda, "get_device_properties", lambda dev: types.SimpleNamespace(multi_processor_count=cus))
    w = {M._BODY_KV: dict(cp=256), M._FACE_KV: dict(cp=512)}
    return types.SimpleNamespace(h2=True, h2dt=H2, dev=types.SimpleNamespace(type="cuda"), compose=compose, pk=types.SimpleNamespace(w=w))


def test_predicate(monkeypatch):
    model, _ = common.product_models(precision="f16x3")
    cx = _as_cuda(monkeypatch)
    assert model._memory_site(cx, 64, T, T) and model._memory_site(cx, 400, T, T)
    assert not model._memory_site(cx, 63, T, T)                 # fewer (clip, head) workgroups than CUs: the composed K / V launch + two-launch sites
    assert not model._memory_site(cx, 64, T, T + 1) and not model._memory_site(cx, 64, 6, 6)       # tail windows
    assert not model._memory_site(_as_cuda(monkeypatch, compose=False), 64, T, T)
    cx.dev.type = "cpu"
    assert not model._memory_site(cx, 64, T, T)
    cx.dev.type = "cuda"
    cx.pk.w[M._FACE_KV]["cp"] = D + 32
    assert not model._memory_site(cx, 64, T, T)                 # a feature width the kernel does not take
    cx.pk.w[M._FACE_KV]["cp"] = 512
    for switch in ("fuse_memory_kv", "fuse_cross_attention"):
        setattr(model, switch, False)
        assert not model._memory_site(cx, 64, T, T)
        setattr(model, switch, True)


def test_stack_sites_get_the_operands_of_the_launches_they_replace(monkeypatch):
    """With the predicates forced on (through the CPU stand-ins): the 8 + 4 stack sites take `ops.qm_attention` with the feature images and the
    composed operands, the three refinement layers keep `ops.q_attention` on their own K / V^T, no K / V launch of a stack remains, and every
    output is bit for bit that of the composed K / V launches + q sites; a tail-sized window falls back."""
    model, _ = common.product_models(precision="f16x3")
    audio, spk, motion, mask = common.window_inputs(1)
    monkeypatch.setattr(type(model), "_fused_cross_attn", lambda self, cx, b, t, tk, d, h: cx.h2 and not self.training and t == tk == T)
    monkeypatch.setattr(type(model), "_memory_site", lambda self, cx, b, t, tk: cx.compose and self.fuse_memory_kv and t == tk == T)
    res, calls, gemms = {}, {}, {}
    with fake_qm_ops.installed(), torch.no_grad():
        for site in (True, False):
            model.fuse_memory_kv = site
            fake_qm_ops.CALLS.clear()
            fake_ops.CALLS.clear()
            res[site] = {k: v.clone() for k, v in model.forward(audio, spk, motion, mask).items() if torch.is_tensor(v)}
            calls[site] = list(fake_qm_ops.CALLS)
            gemms[site] = fake_ops.CALLS.count("gemm")
        model.fuse_memory_kv = True
        fake_qm_ops.CALLS.clear()
        short = model.forward(audio[:, :6 * 533], spk, motion[:, :6], mask[:, :6])
        assert not fake_qm_ops.CALLS and all(torch.isfinite(v).all() for v in short.values() if torch.is_tensor(v))
    nc, nf = M.spec.N_CROSS_LAYERS, M.spec.N_FACE_LAYERS
    qm = [c for c in calls[True] if c[0] == "qm_attention"]
    assert sorted(c[1:] for c in qm) == sorted([((T, 256), 256, nc, i) for i in range(nc)] + [((T, 512), 512, nf, i) for i in range(nf)])
    assert [c for c in calls[True] if c[0] == "q_attention"] == [("q_attention", (T, D), D)] * 3
    assert len(calls[False]) == nc + nf + 3 and all(c[0] == "q_attention" for c in calls[False])
    # the stand-in restates each site as K / V launch + q projection: 2 launches x 12 sites in place of 2 K / V launches + 12 q projections... of which the
    # q projections live inside both stand-ins: the forward itself issues exactly two contractions fewer
    assert gemms[True] - 2 * len(qm) == gemms[False] - 2 - (nc + nf), gemms
    for k, v in res[True].items():
        assert torch.equal(v, res[False][k]), k


def test_entry_points_refuse_before_any_launch():
    lib = _lib.load()
    arr = (_lib.QmAttentionProblem * 5)()
    assert lib.emage_qm_attention(H2, None, T, T, D, H, None) == -1
    assert lib.emage_qm_attention(H2, arr, T, T, D, H, None) == -1                   # null pointers
    assert lib.emage_qm_attention_grouped(H2, arr, 0, T, T, D, H, None) == -1
    assert lib.emage_qm_attention_grouped(H2, arr, 5, T, T, D, H, None) == -1
    p = arr[0]
    p.A = p.W = p.bias = p.mem = p.Wkv = p.bias_kv = p.out = 4096                    # aligned, never dereferenced: every call below is refused
    p.lda = p.ldo = D
    p.ldm = p.km = 256
    p.kv_layers, p.kv_layer, p.B, p.a_scale, p.w_scale, p.wkv_scale = 8, 3, 1, 16.0, 1.0, 1.0
    assert lib.emage_qm_attention(H2, arr, T, 32, D, H, None) == -1 and lib.emage_qm_attention(F16X3, arr, T, T, D, H, None) == -1
    assert lib.emage_qm_attention(H2, arr, 32, T, D, H, None) == -1 and lib.emage_qm_attention(H2, arr, T, T, 512, H, None) == -1
    assert lib.emage_qm_attention(H2, arr, T, T, D, 8, None) == -1
    for field, bad in (("km", 0), ("km", 48), ("km", D + 32), ("ldm", 248), ("ldm", 260), ("kv_layers", 0), ("kv_layers", 65), ("kv_layer", 8),
                       ("kv_layer", -1), ("wkv_scale", 0.0), ("w_scale", 0.0), ("lda", D + 4), ("ldo", D - 8), ("A", 4100), ("mem", 4104),
                       ("Wkv", 4100), ("bias_kv", 4100), ("mem", None), ("Wkv", None), ("bias_kv", None), ("B", 1 << 20), ("B", 0)):
        keep = getattr(p, field)
        setattr(p, field, bad)
        assert lib.emage_qm_attention(H2, arr, T, T, D, H, None) == -1, (field, bad)
        setattr(p, field, keep)


def test_problem_table_words():
    """The words `qm_attention_grouped` carries, against a structure set by hand (as tests/test_problem_tables_host.py does for the others)."""
    ints = ("A", "W", "bias", "ln_stats", "ln_c", "mem", "Wkv", "bias_kv", "out", "lda", "ldm", "km", "kv_layers", "kv_layer", "ldo", "B")
    assert ops._QM_TABLE.struct is _lib.QmAttentionProblem and ops._QM_TABLE.ints == ints
    assert ops._QM_TABLE.floats == ("a_scale", "w_scale", "wkv_scale", "ln_eps")
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32)
    raws, entries, tensors = [], [], []
    for full in (True, False):
        a, w, bias, out = f32(2 * T, 800), f32(D, D), f32(D), f32(2 * T, 776)
        mem, wkv, bkv = f32(6 * T, 264)[T:3 * T], f32(2 * 8 * D, 256), f32(2 * 8 * D)
        ln_stats, ln_c = (f32(2 * T, 24, 2), f32(D)) if full else (None, None)
        args = (H2, a, w, bias, ln_stats, ln_c, mem, wkv, bkv, out, 2, 256, 8, 5, 4096.0, 2048.0, 16.0, 1e-5 if full else 0.0)
        pt = lambda t: None if t is None else t.data_ptr()
        s = _lib.QmAttentionProblem(A=pt(a), W=pt(w), bias=pt(bias), ln_stats=pt(ln_stats), ln_c=pt(ln_c), mem=pt(mem), Wkv=pt(wkv), bias_kv=pt(bkv),
                                    out=pt(out), lda=800, ldm=264, km=256, kv_layers=8, kv_layer=5, ldo=776, B=2, a_scale=16.0, w_scale=4096.0,
                                    wkv_scale=2048.0, ln_eps=1e-5 if full else 0.0)
        assert mem.data_ptr() == mem._base.data_ptr() + T * 264 * 4
        raws.append(bytes(s))
        entries.append(("qm_attention", None, args, {}))
        tensors += [t for t in args[1:10] if torch.is_tensor(t)]
        arr, n = ops._QM_TABLE.array(*ops._QM_TABLE.pack(ops._qm_fields(*args)))
        assert n == 1 and bytes(arr) == raws[-1]
    dtype, got, desc, scales = ops._pack_entries(ops._QM_TABLE, ops._qm_fields, entries)
    assert dtype == H2 and len(desc) == 2 * len(ints) and len(scales) == 8 and all(type(v) is int for v in desc)
    arr, n = ops._QM_TABLE.array(desc, scales)
    assert n == 2 and bytes(arr) == raws[0] + raws[1] and arr[1].ln_stats is None and arr[0].ln_stats is not None
    assert len(got) == len(tensors) and all(x is y for x, y in zip(got, tensors))
    assert "qm_attention" in ops._GROUPED


def test_sites_are_traced_with_their_family_and_grouped_by_operator():
    """A `qm_attention` call is recorded under `q_attention` (what trace hooks and launch logs see) with its own name in meta["op"]; heads of
    the two operators at one lock-step round go out as one grouped call EACH."""
    issued = []
    ls = ops.Lockstep(True)
    ls._issue = lambda e: issued.append(("one", ops._operator(e)))
    ls._issue_group = lambda es: issued.append(("group", ops._operator(es[0]), len(es)))
    qm = lambda: ("q_attention", None, (H2,), {"op": "qm_attention"})
    q = lambda: ("q_attention", None, (H2,), {})
    ls.chains = [[qm(), q()], [qm()], [q(), qm()], [q()]]
    assert ls._groupable(qm()) and ops._operator(qm()) == "qm_attention" and ops._operator(q()) == "q_attention"
    ls.run()
    assert issued == [("group", "qm_attention", 2), ("group", "q_attention", 2), ("one", "q_attention"), ("one", "qm_attention")]
    rec = ops.Lockstep(True)
    ops._RECORDER[0] = rec
    try:
        with rec.chain():
            ops._qm_attention(H2)                    # recorded, not launched: the arguments are not looked at
    finally:
        ops._RECORDER[0] = None
    (e,) = rec.chains[0]
    assert e[0] == "q_attention" and e[3]["op"] == "qm_attention" and e[1] is ops._qm_attention.op


def test_hoisted_features_without_kv_serve_a_batch_that_keeps_the_launches(monkeypatch):
    """Features hoisted for a batch large enough for the sites (no K / V^T computed) and consumed clip by clip by forwards that are not: the
    forward issues the composed K / V launch itself."""
    model, _ = common.product_models(precision="f16x3")
    audio, spk, motion, mask = common.window_inputs(2)
    monkeypatch.setattr(type(model), "_memory_site", lambda self, cx, b, t, tk: cx.compose and b >= 2 and t == tk == T)
    with fake_qm_ops.installed(), torch.no_grad():
        cx = M._Ctx(model._engine())
        with M.Fork(torch.device("cpu"), 3, model.concurrent) as fk:
            feats = model._audio_features(cx, audio, 2, T, True, fk, 1, 2)
        assert feats["body"].k is None and feats["body"].vt is None and feats["body"].img.shape == (2 * T, model.config.audio_f)
        for i in range(2):
            one = model._feats_of_clips(feats, i, 1, T)
            assert one["body"].k is None and one["body"].img.shape[0] == T and one["memcat"].shape[0] == T
            one["memcat"] = one["memcat"].clone()                        # the forward writes the body hints into its columns
            got = model.forward(audio[i:i + 1], spk[i:i + 1], motion[i:i + 1], mask[i:i + 1], _audio_feats=one)
            ref = model.forward(audio[i:i + 1], spk[i:i + 1], motion[i:i + 1], mask[i:i + 1])
            for k, v in ref.items():
                if torch.is_tensor(v):
                    assert float((v - got[k]).abs().max()) < 1e-5, (i, k)
    assert not fake_qm_ops.CALLS
