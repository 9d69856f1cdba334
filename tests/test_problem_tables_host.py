"""The problem tables of the three grouped operators (ops._ProblemTable: gemm_grouped, qkv_attention_grouped, q_attention_grouped) against
the field orders, packed bytes and tensor lists their hand-written predecessors produced, written out here as literals.  No GPU and no
library: the tensors are CPU tensors (distinct `data_ptr()`s), the structures are filled and compared as bytes."""
import torch

from pantomatrix_amd import _lib, ops
from pantomatrix_amd._lib import H2

GEMM_INTS = ("A", "W", "bias", "slope", "res", "out", "out_f32", "out_t", "lda", "ldr", "res_is_f32", "res_first", "ldo", "n_store", "ldf",
             "t_col0", "t_rows", "t_ld", "M", "N", "Cp", "taps", "stride", "pad", "Lin", "Lout",
             "ln_stats", "ln_c", "rs_stats", "rs_gamma", "rs_beta", "st_out", "ln_np", "rs_np", "sk_ws", "sk_ws_bytes", "sk_count", "sk_tiles")
QKV_INTS = ("A", "W", "bias", "ln_stats", "ln_c", "out", "lda", "ldo", "B")
QA_INTS = ("A", "W", "bias", "ln_stats", "ln_c", "k", "vt", "out", "lda", "ldk", "ldvt", "vt_rows", "ldo", "B")
SCALES = ("a_scale", "w_scale", "ln_eps")

M, D = 8, 768


def f32(*shape):
    return torch.zeros(*shape, dtype=torch.float32)


def by_hand(struct, **fields):
    s = struct()
    assert set(fields) == {n for n, _t in struct._fields_}
    for k, v in fields.items():
        setattr(s, k, v)
    return bytes(s)


def entry(name, *args):
    return (name, None, args, {})


def gemm_case(full):
    """All 33 positional arguments of emage::gemm (full: every optional tensor present; else every optional tensor None) and the structure
    they stand for, field by field."""
    a, w, out = f32(M, 800), f32(D, D), f32(M, 776)
    o = (lambda t: t) if full else (lambda t: None)
    bias, slope, res, out_f32, out_t = o(f32(D)), o(f32(D)), o(f32(M, 784)), o(f32(M, 792)), o(f32(3, D, 64))
    ln_stats, ln_c, rs_stats, rs_gamma, rs_beta, st_out = o(f32(M, 24, 2)), o(f32(D)), o(f32(M + 1, 16, 2)), o(f32(D)), o(f32(D)), o(f32(M, 24, 2))
    sk_ws, sk_count = o(f32(1000)), o(torch.zeros(50, dtype=torch.int32))
    args = (H2, a, w, bias, slope, res, out, out_f32, out_t, D, 768, 770, 512, 5, True, 3, 2, 1, 16, 8, M, 4096.0, 16.0, False,
            ln_stats, ln_c, rs_stats, rs_gamma, rs_beta, st_out, 1e-5, sk_ws, sk_count)
    assert len(args) == 33
    p = lambda t: None if t is None else t.data_ptr()
    raw = by_hand(_lib.GemmProblem, A=p(a), W=p(w), bias=p(bias), slope=p(slope), res=p(res), out=p(out), out_f32=p(out_f32), out_t=p(out_t),
                  lda=800, ldr=784 if full else 0, res_is_f32=1 if full else 0, res_first=1, ldo=776, n_store=770, ldf=792 if full else 0,
                  t_col0=512, t_rows=5, t_ld=64 if full else 0, M=M, N=D, Cp=768, taps=3, stride=2, pad=1, Lin=16, Lout=8,
                  a_scale=16.0, w_scale=4096.0, ln_stats=p(ln_stats), ln_c=p(ln_c), rs_stats=p(rs_stats), rs_gamma=p(rs_gamma), rs_beta=p(rs_beta),
                  st_out=p(st_out), ln_np=24 if full else 0, rs_np=16 if full else 0, ln_eps=1e-5, sk_ws=p(sk_ws), sk_ws_bytes=4000 if full else 0,
                  sk_count=p(sk_count), sk_tiles=50 if full else 0)
    old_tensors = [t for t in args[1:9] + args[24:30] + args[31:33] if torch.is_tensor(t)]
    return entry("gemm", *args), raw, old_tensors


def qkv_case(full):
    a, w, bias, out = f32(2 * 64, 800), f32(3 * D, D), f32(3 * D), f32(2 * 64, 776)
    ln_stats, ln_c = (f32(2 * 64, 24, 2), f32(3 * D)) if full else (None, None)
    args = (H2, a, w, bias, ln_stats, ln_c, out, 2, 4096.0, 16.0, 1e-5 if full else 0.0)
    p = lambda t: None if t is None else t.data_ptr()
    raw = by_hand(_lib.QkvAttentionProblem, A=p(a), W=p(w), bias=p(bias), ln_stats=p(ln_stats), ln_c=p(ln_c), out=p(out), lda=800, ldo=776, B=2,
                  a_scale=16.0, w_scale=4096.0, ln_eps=1e-5 if full else 0.0)
    return entry("qkv_attention", *args), raw, [t for t in args[1:7] if torch.is_tensor(t)]


def qa_case(full):
    a, w, bias, out = f32(2 * 64, 800), f32(D, D), f32(D), f32(2 * 64, 776)
    k, vt = f32(2 * 64, 784), f32(2, 2 * D, 96)[:, D:]
    ln_stats, ln_c = (f32(2 * 64, 24, 2), f32(D)) if full else (None, None)
    args = (H2, a, w, bias, ln_stats, ln_c, k, vt, 2 * D, out, 2, 4096.0, 16.0, 1e-5 if full else 0.0)
    p = lambda t: None if t is None else t.data_ptr()
    raw = by_hand(_lib.QAttentionProblem, A=p(a), W=p(w), bias=p(bias), ln_stats=p(ln_stats), ln_c=p(ln_c), k=p(k), vt=p(vt), out=p(out),
                  lda=800, ldk=784, ldvt=96, vt_rows=2 * D, ldo=776, B=2, a_scale=16.0, w_scale=4096.0, ln_eps=1e-5 if full else 0.0)
    return entry("q_attention", *args), raw, [t for t in args[1:10] if torch.is_tensor(t)]


KINDS = {"gemm": (ops._GEMM_TABLE, ops._gemm_fields, gemm_case, _lib.GemmProblem, GEMM_INTS),
         "qkv_attention": (ops._QKV_TABLE, ops._qkv_fields, qkv_case, _lib.QkvAttentionProblem, QKV_INTS),
         "q_attention": (ops._QA_TABLE, ops._qa_fields, qa_case, _lib.QAttentionProblem, QA_INTS)}

# the pointer fields of the cases built with full=False (every optional tensor None)
NULL_WHEN_BARE = {"gemm": ("bias", "slope", "res", "out_f32", "out_t", "ln_stats", "ln_c", "rs_stats", "rs_gamma", "rs_beta", "st_out", "sk_ws", "sk_count"),
                  "qkv_attention": ("ln_stats", "ln_c"), "q_attention": ("ln_stats", "ln_c")}


def test_word_orders_are_the_hand_written_ones():
    for kind, (table, _fields, _case, struct, ints) in KINDS.items():
        assert table.struct is struct, kind
        assert table.ints == ints, kind
        assert table.floats == SCALES, kind


def test_packed_problems_equal_structures_set_by_hand():
    for kind, (table, fields, case, struct, ints) in KINDS.items():
        (e_full, raw_full, _), (e_none, raw_none, _) = case(True), case(False)
        assert raw_full != raw_none
        # one problem, as the single-problem operators pack it
        arr, n = table.array(*table.pack(fields(*e_full[2])))
        assert n == 1 and bytes(arr) == raw_full, kind
        # two problems from recorded entries, as the grouped operators receive them
        dtype, _tensors, desc, scales = ops._pack_entries(table, fields, [e_none, e_full])
        assert dtype == H2 and len(desc) == 2 * len(ints) and len(scales) == 2 * len(SCALES), kind
        assert all(type(v) is int for v in desc) and all(type(v) is float for v in scales), kind
        arr, n = table.array(desc, scales)
        assert n == 2 and bytes(arr) == raw_none + raw_full, kind
        for name, ctype in struct._fields_:                  # None tensors are null pointers, and nothing else is
            if ctype is _lib._p:
                assert (getattr(arr[0], name) is None) == (name in NULL_WHEN_BARE[kind]), (kind, name)
                assert getattr(arr[1], name) is not None, (kind, name)


def test_tensor_lists_are_the_old_positional_slices():
    for kind, (table, fields, case, _struct, _ints) in KINDS.items():
        want = []
        entries = []
        for full in (True, False, True):
            e, _raw, old = case(full)
            entries.append(e)
            want += old
        got = ops._pack_entries(table, fields, entries)[1]
        assert len(got) == len(want) and all(g is w for g, w in zip(got, want)), kind
    assert len(gemm_case(True)[2]) == 16 and len(gemm_case(False)[2]) == 3
    assert len(qkv_case(True)[2]) == 6 and len(qa_case(False)[2]) == 6


def test_six_self_attention_sites_go_out_as_four_and_two(monkeypatch):
    calls = []
    monkeypatch.setattr(ops._qkv_attention_grouped, "op", lambda dtype, tensors, desc, scales: calls.append((dtype, tensors, desc, scales)))
    cases = [qkv_case(i % 2 == 0) for i in range(6)]
    entries = [c[0] for c in cases]
    ls = ops.Lockstep(True)
    ls._issue_group(entries)
    assert ops._QKV_MAXG == 4
    assert [len(c[2]) // len(QKV_INTS) for c in calls] == [4, 2]
    assert [len(c[3]) for c in calls] == [12, 6]
    assert all(c[0] == H2 for c in calls)
    arrs = [ops._QKV_TABLE.array(c[2], c[3])[0] for c in calls]
    assert bytes(arrs[0]) + bytes(arrs[1]) == b"".join(c[1] for c in cases)
    got, want = [t for c in calls for t in c[1]], [t for c in cases for t in c[2]]
    assert len(got) == len(want) == 3 * 6 + 3 * 4 and all(g is w for g, w in zip(got, want))
    assert ls.launches == [("group", 6)] and ls.groups == [entries]
