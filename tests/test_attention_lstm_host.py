"""The case table of tests/attention_lstm_cases.py run on the CPU, through the fp32 stand-ins of tests/fake_ops.py and through torch's own fp32
code (scaled_dot_product_attention; torch.nn.LSTMCell behind the step signatures; torch.nn.LSTM in fp32 is one of the two yardsticks inside
`layer_case`): correct fp32 code passes every tolerance the GPU test applies, every wrong reference is rejected, the peaked cases have the
stated score margin in float64 (asserted inside `check_attention`), and the index arithmetic of the V^T chunks is what the kernel's zero-operand rule assumes.  No GPU."""
import pytest
import torch

import attention_lstm_cases as ac
import fake_ops as F
from pantomatrix_amd import ops
from pantomatrix_amd._lib import F16X3


@pytest.mark.parametrize("name,tk,tq,b,h,kind", ac.ATT_CASES)
def test_attention(name, tk, tq, b, h, kind):
    ac.check_attention(F, name, tk, tq, b, h, kind)


@pytest.mark.parametrize("name,tk,tq,b,h", ac.DROP_CASES)
def test_attention_dropout(name, tk, tq, b, h):
    ac.check_attention_dropout(F, name, tk, tq, b, h)


class TorchAttention:
    """torch's own fp32 attention on the CPU behind the `attention` / `attention_dropout` signatures (BF16: the stored bf16 operands in fp32
    arithmetic, the result rounded to bf16 by the copy into `out`; H2 through the fake's image writer)."""

    @staticmethod
    def _sdpa(q, k, vt, vt_rows, b, h, tq, tk, hd, pmask=None):
        tp = vt.shape[-1]
        qf = torch.as_strided(q, (b * tq, h * hd), (q.stride(0), 1)).float().view(b, tq, h, hd).transpose(1, 2)
        kf = torch.as_strided(k, (b * tk, h * hd), (k.stride(0), 1)).float().view(b, tk, h, hd).transpose(1, 2)
        vf = torch.as_strided(vt, (b, h * hd, tp), (vt_rows * tp, tp, 1))[:, :, :tk].float().reshape(b, h, hd, tk).transpose(2, 3)
        if pmask is None:
            o = torch.nn.functional.scaled_dot_product_attention(qf, kf, vf)
        else:
            o = (torch.softmax(qf @ kf.transpose(-1, -2) / hd ** 0.5, -1) * pmask) @ vf
        return o.transpose(1, 2).reshape(b * tq, h * hd)

    @classmethod
    def attention(cls, dtype, q, k, vt, vt_rows, out, b, h, tq, tk, hd):
        o = cls._sdpa(q, k, vt, vt_rows, b, h, tq, tk, hd)
        if dtype == ac.H2:
            F.h2_store(out, o)
        else:
            out.copy_(o)

    @classmethod
    def attention_dropout(cls, dtype, q, k, vt, vt_rows, out, b, h, tq, tk, hd, pmask):
        out.copy_(cls._sdpa(q, k, vt, vt_rows, b, h, tq, tk, hd, pmask))


@pytest.mark.parametrize("name,tk,tq,b,h,kind", ac.ATT_CASES)
def test_attention_torch_fp32(name, tk, tq, b, h, kind):
    ac.check_attention(TorchAttention, name, tk, tq, b, h, kind)


@pytest.mark.parametrize("name,tk,tq,b,h", ac.DROP_CASES)
def test_attention_dropout_torch_fp32(name, tk, tq, b, h):
    ac.check_attention_dropout(TorchAttention, name, tk, tq, b, h)


def test_vt_chunks_past_ldvt():
    """Which V^T chunk covers which columns, for every Tk: only the NT = 8 path with ldvt = 96 (Tk in 65..96) has chunks past the row — fp32
    chunks 6 and 7 (columns 96..127), bf16 chunk 3 (96..127) — those are exactly the chunks the kernel replaces by a zero operand, no loaded
    chunk reaches past ldvt, and no chunk that holds a real key is dropped."""
    for name in ("f32", "bf16"):
        past = {}
        for tk in range(1, 129):
            ldvt = ops.round_up(tk, 32)
            for c, first, last in ac.vt_chunk_columns(name, tk):
                assert first % 4 == 0 and last < 16 * ac.att_nt(tk)
                if last >= ldvt:
                    past.setdefault(tk, []).append(c)
                    assert first >= ldvt and first >= tk                 # wholly past the row: it holds no key
                assert ac.vt_chunk_is_loaded(name, tk, c, ldvt) == (last < ldvt), (name, tk, c)
                assert ac.vt_chunk_is_loaded(name, tk, c, 128)           # a 128-wide row: every chunk is loaded
        assert sorted(past) == list(range(65, 97))
        assert all(cs == ([3] if name == "bf16" else [6, 7]) for cs in past.values())
    assert ac.ATT_READS_PAST_LDVT in ac.ATT_CASES and 65 <= ac.ATT_READS_PAST_LDVT[1] <= 96


@pytest.mark.parametrize("name,b,hid,paired", ac.LSTM_STEP_CASES)
def test_lstm_steps(name, b, hid, paired):
    ac.check_lstm_steps(F, name, b, hid, paired)


@pytest.mark.parametrize("name", list(ac.LSTM_DTYPES))
def test_lstm_gate_functions(name):
    ac.check_lstm_gate_functions(F, name)


class TorchLstm:
    """torch.nn.LSTMCell in fp32 on the CPU behind the `lstm_step` / `lstm_step_pair` signatures.  The operands arrive in the product's layout
    (rows 4u + g, for F16X3 as the packed split image of W * w_scale): they are put back into torch's [i | f | g | o] blocks, the cell's
    weight_ih is the identity and its biases zero, so it is given exactly the gates_x the kernels get."""

    @staticmethod
    def lstm_step(dtype, h_prev, w_hh, gates_x, cstate, h_out, *, w_scale=1.0, a_scale=None):
        b, hid = cstate.shape
        if dtype == F16X3:
            hi, lo = F.unsplit_f16_weights(w_hh, 4 * hid, hid)
            w_hh = (hi + lo) / w_scale
        cell = torch.nn.LSTMCell(4 * hid, hid)
        with torch.no_grad():
            cell.weight_hh.copy_(w_hh.view(hid, 4, hid).transpose(0, 1).reshape(4 * hid, hid))
            cell.weight_ih.copy_(torch.eye(4 * hid))
            cell.bias_ih.zero_()
            cell.bias_hh.zero_()
            h, c = cell(gates_x.view(b, hid, 4).transpose(1, 2).reshape(b, 4 * hid), (h_prev.contiguous(), cstate.contiguous()))
        cstate.copy_(c)
        h_out.copy_(h)

    @classmethod
    def lstm_step_pair(cls, dtype, fwd, bwd, *, a_scale=None):
        for h_prev, w_hh, gates_x, cstate, h_out, w_scale in (fwd, bwd):
            cls.lstm_step(dtype, h_prev, w_hh, gates_x, cstate, h_out, w_scale=w_scale)


@pytest.mark.parametrize("name,b,hid,paired", ac.LSTM_STEP_CASES)
def test_lstm_steps_torch_fp32(name, b, hid, paired):
    ac.check_lstm_steps(TorchLstm, name, b, hid, paired)


@pytest.mark.parametrize("name", list(ac.LSTM_DTYPES))
def test_lstm_gate_functions_torch_fp32(name):
    ac.check_lstm_gate_functions(TorchLstm, name)


def test_product_regroup_is_a_permutation():
    """The regrouping read off `_pack_lstm` moves torch's row g H + u to row 4 u + g in both directions — stated here once, independently."""
    hid = 64
    w = [torch.arange(4 * hid * hid, dtype=torch.float32).view(4 * hid, hid) + d for d in range(2)]
    wp, idx = ac.product_regroup(w)
    for d in range(2):
        assert torch.equal(wp[d].view(hid, 4, hid), w[d].view(4, hid, hid).transpose(0, 1))
        assert torch.equal(idx[4 * hid * d:4 * hid * (d + 1)].view(hid, 4), torch.arange(4 * hid).view(4, hid).t())


@pytest.mark.parametrize("hid,b,t", ac.LAYER_CASES)
def test_lstm_layer(hid, b, t):
    """fake_ops.lstm_layer is one of the two fp32 yardsticks, so it passes by construction; what this shows is that the two restatements
    (the step arithmetic in fp32 torch, torch.nn.LSTM in fp32) agree with float64 to the same order, that the written-out float64 cell is
    torch.nn.LSTM, and that the wrong references are rejected at 4 x that error."""
    err32, err = ac.check_lstm_layer(F, hid, b, t)
    case = ac.layer_case(hid, b, t)
    assert err <= err32 and max(case["err_fake"], case["err_torch"]) <= 4 * max(min(case["err_fake"], case["err_torch"]), ac.LAYER_FLOOR / 4)


def test_softmax2_mix():
    ac.check_softmax2_mix(F)


def test_softmax2_mix_torch_fp32():
    class T:
        @staticmethod
        def softmax2_mix(sel, c1, c2, out):
            out.copy_((torch.softmax(sel[:, :2], 1).unsqueeze(-1) * torch.stack([c1, c2], 1)).sum(1))
    ac.check_softmax2_mix(T)
