"""Forward attention (csrc/attention.hip, attn_tile.h), the LSTM cell (EPI_LSTM of csrc/gemm_tile.h, csrc/lstm.hip, csrc/lstmseq.hip) and
softmax2_mix, called through pantomatrix_amd.ops on the MI355X against float64 references built from the stored operands: peaked and shifted
softmaxes, every Tk / Tq at a dispatch, tile or wave boundary, V^T padding that is not zero, V^T rows followed by NaN, gate pre-activations from
1e-4 to +-1e4, the recurrence against torch.nn.LSTM in float64 over up to 415 steps.  The cases, references, tolerances and wrong references live in
tests/attention_lstm_cases.py (shared with tests/test_attention_lstm_host.py); the conventions are those of test_forward_kernels_gpu.py.

Largest error of each operation on an MI355X, its fraction of the tolerance at that case, and the case ((Tk, Tq, B, H, kind) for attention, (B, H)
for the steps); then the largest fraction of the tolerance over all cases.  The accumulation terms of the tolerances are the any-order worst case
(n - 1) u sum|terms|, which is why fp32-grade results sit at a few percent of them; every comparison prints its own figure:
    attention f32            1.186e-04   0.016   (33, 65, 2, 1, shifted)      largest fraction 0.037  (17, 16, 2, 3, qzero)
    attention bf16           1.264e-02   0.383   (16, 15, 1, 1, shifted)      largest fraction 0.632  (31, 63, 1, 1, normal)
    attention f16x3          7.469e-05   0.003   (33, 65, 2, 1, shifted)      largest fraction 0.013  (17, 16, 2, 3, qzero)
    attention h2             1.053e-04   0.003   (33, 65, 2, 1, shifted)      largest fraction 0.017  (17, 16, 2, 3, qzero)
    attention_dropout f32    1.157e-06   0.004   (15, 17, 2, 3)
    attention_dropout f16x3  9.120e-07   0.001   (33, 16, 1, 1)
    lstm_step h f32          8.081e-07   0.127   (130, 256)                   largest fraction 0.152  (64, 64)
    lstm_step h f16x3        4.849e-07   0.194   (63, 512)                    largest fraction 0.203  (65, 512)
    lstm_step c f32          2.416e-06   0.115   (130, 512)
    lstm_step c f16x3        2.249e-06   0.083   (130, 512)
    lstm_step_pair           the same four rows, figure for figure: every case gives the same errors through either entry point
    sigmoid alone, f32       6.634e-08   0.278   = 1.1 EPS32 (bound 4 EPS32)
    sigmoid alone, f16x3     8.767e-08   0.368   = 1.5 EPS32 (bound 4 EPS32; the fast form rcp(1 + exp2(.)))
    tanh alone, f32          6.307e-08   0.265   = 1.1 EPS32 (bound 4 EPS32)
    tanh alone, f16x3        1.933e-07   0.360   = 3.2 EPS32 (bound 9 EPS32; the fast form 1 - 2 rcp(1 + exp2(.)): absolute, so 1e-3 relative at x = 1e-4)
    softmax2_mix             1.375e-07   0.155   (5 EPS32 per weight)
On the parent commit the 12 attention cases with Tk in {65, 80, 96} (all four dtypes) return NaN: the V^T chunks of keys [96, 128) were loaded from the
next row of the buffer, which is NaN here (see ATT_READS_PAST_LDVT and the CHANGELOG).

lstm_layer against torch.nn.LSTM in float64, largest error over the (B, T, 2H) output.  The fp32 column is the larger error of the two fp32 restatements
on the CPU (fake_ops.lstm_layer, torch.nn.LSTM in fp32), computed inside the test; the kernel may be 4 x that, floor 8 EPS32 = 4.8e-7.  The error does
not grow with T: with N(0, 1 / H) recurrent weights the cell is contractive.
    H     B    T      fp32 restatement   kernel (MI355X)
    256   1    1      7.441e-08          1.569e-07
    256   3    2      1.069e-07          1.505e-07
    256   65   5      2.632e-07          2.471e-07
    256   17   33     2.160e-07          2.611e-07
    256   3    415    3.099e-07          2.818e-07
    512   1    1      7.037e-08          1.365e-07
    512   3    2      1.610e-07          1.860e-07
    512   65   5      3.165e-07          2.743e-07
    512   17   33     4.149e-07          3.013e-07"""
import pytest

import attention_lstm_cases as ac
from pantomatrix_amd import ops
from pantomatrix_amd._lib import F16X3

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,tk,tq,b,h,kind", ac.ATT_CASES)
def test_attention(name, tk, tq, b, h, kind):
    ac.check_attention(ops, name, tk, tq, b, h, kind)


@pytest.mark.parametrize("name,tk,tq,b,h", ac.DROP_CASES)
def test_attention_dropout(name, tk, tq, b, h):
    ac.check_attention_dropout(ops, name, tk, tq, b, h)


@pytest.mark.parametrize("name,b,hid,paired", ac.LSTM_STEP_CASES)
def test_lstm_steps(name, b, hid, paired):
    ac.check_lstm_steps(ops, name, b, hid, paired)


@pytest.mark.parametrize("name", list(ac.LSTM_DTYPES))
def test_lstm_gate_functions(name):
    ac.check_lstm_gate_functions(ops, name)


@pytest.mark.parametrize("hid,b,t", ac.LAYER_CASES)
def test_lstm_layer(hid, b, t):
    if not ops.lstm_layer_supported(F16X3, hid):
        pytest.skip("the device cannot hold the persistent recurrence's blocks")
    ac.check_lstm_layer(ops, hid, b, t)


def test_softmax2_mix():
    ac.check_softmax2_mix(ops)
