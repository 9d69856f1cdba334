"""The forward reductions, LayerNorm, optimizer and rotation kernels that training and decode depend on (csrc/train.hip, optim.hip, elementwise.hip /
ln_row.h, vq.hip, motion.hip / rot_math.h), each called through pantomatrix_amd.ops on the MI355X against a float64 reference of the
mathematical operation on the CPU, at the shapes where such kernels go wrong: lane, chunk and grid-stride boundaries, strided views,
constant rows, large means, branch thresholds.  The cases, references, tolerances and wrong references live in tests/forward_cases.py
(shared with tests/test_forward_kernels_host.py, which runs them through fp32 torch on the CPU); the conventions are those of
test_backward_kernels_gpu.py.

Largest error of each operation on an MI355X (absolute, as a fraction of the reference's scale, and the case it occurred in; each comparison
prints its own):
    layernorm y_f32          1.391e-04   2.3e-05   M=1 C=768 (the mean-1e3 row; the same figure for F32, BF16 and H2; N(0,1) rows stay below 1e-6)
    bn_stats mean            3.492e-10   3.6e-08   M=64 C=1
    bn_stats var             2.804e-10   2.8e-06   M=257 C=1 (mean 1e3, std 1e-2: a third of the 2^-50 (mean^2 + var) term)
    bn_stats running_mean    9.678e-06   9.5e-08   M=1025 C=63, momentum 0.1
    bn_stats running_var     2.829e-10   2.9e-06   M=257 C=1, momentum 1
    bn_apply                 1.713e-06   1.8e-07   130 x 65, no shortcut
    mse_loss                 1.110e-07   2.6e-08   1 x 1
    nll_loss                 1.728e-06   6.0e-09   130 x 256
    col_sum                  6.559e-08   2.4e-07   1025 x 1 with y; deferred finalize bit-identical everywhere
    transpose, mul_add       exact
    adam param               7.936e-08   1.4e-07   n=1, step 3, weight decay 0.01 (all three entry points)
    adam exp_avg             5.005e-08   1.4e-07   adam_multi n=4095, step 10 002
    adam exp_avg_sq          3.776e-09   2.0e-07   n=4097; against the exact betas (0.9, 0.999): 1.3e-05 of the scale, bound 3e-05 per step
    argmax_logsoftmax        0 of 162 rows differ
    axis_angle_to_rot6d      3.691e-07   3.7e-07   angle 3 pi
    velocity_to_position     1.763e-05   2.5e-06   B=23 T=5121 against float64; bit-equal to the sequential fp32 recurrence everywhere
    merge_parts              at most 0.25 of the per-slot tolerance (aa and motion layouts); copies exact

rot6d -> axis-angle, error in matrix space per input class (176 x 4 regular inputs pooled by angle; 176 per degenerate kind).  The fp32 oracle
column is the CPU run of oracle/emage_oracle.py in fp32 against float64; the kernel may be 4 x that (floor 8 EPS32 = 4.8e-7).  The reference
algorithm itself loses the rotation at angle pi (the signs of the quaternion's vector part come from rounding noise) and half its digits at
small angles (sqrt(1 + m00 - m11 - m22) of a difference of ~1e-7), which is why the bound is per class:
    class            fp32 oracle     kernel (MI355X)
    angle 0          0.000e+00       0.000e+00
    angle 1e-8       1.000e-08       1.000e-08
    angle 9e-7       9.000e-07       9.000e-07
    angle 1.1e-6     1.100e-06       1.100e-06
    angle 1e-3       4.229e-04       4.231e-04
    angle pi/2       8.416e-07       8.450e-07
    angle pi-1e-3    4.229e-04       4.231e-04
    angle pi         1.775e+00       1.775e+00
    angle pi+1e-3    4.229e-04       4.231e-04
    angle 2pi-1e-3   4.229e-04       4.231e-04
    angle 3pi        1.775e+00       1.775e+00
    a1 = 0           4.738e-05       4.738e-05
    a2 || a1         2.000e+00       2.000e+00
    all zero         9.082e-08       2.839e-08
Every degenerate input gives a finite result (176 of 176 in each kind)."""
import pytest
import torch

import forward_cases as fc
from pantomatrix_amd import ops
from pantomatrix_amd._lib import F32, EmageKernelError

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("c", fc.LN_C)
@pytest.mark.parametrize("name", list(fc.LN_DTYPES))
def test_layernorm(name, c):
    fc.check_layernorm(ops, name, c)


@pytest.mark.parametrize("which", list(fc.LN_REFUSED))
def test_layernorm_refuses(which):
    x, gamma, beta, y = fc.layernorm_refused_args(DEV, which)
    with pytest.raises(EmageKernelError):
        ops.layernorm(F32, x, gamma, beta, 1e-5, None, y, None)


@pytest.mark.parametrize("m", fc.BN_M)
def test_bn_stats(m):
    fc.check_bn_stats(ops, m)


@pytest.mark.parametrize("m,c,mode,slope", fc.BN_APPLY_CASES)
def test_bn_apply(m, c, mode, slope):
    fc.check_bn_apply(ops, m, c, mode, slope)


@pytest.mark.parametrize("m,c", fc.MSE_SHAPES)
def test_mse_loss(m, c):
    fc.check_mse_loss(ops, m, c)


@pytest.mark.parametrize("m,k", fc.NLL_SHAPES)
def test_nll_loss(m, k):
    logits, index, loss, ws = fc.check_nll_loss(ops, m, k)
    if m == 130:                     # a class index outside [0, K) raises the sticky flag of the workspace
        bad = index.clone()
        bad[77] = k
        ops.nll_loss(logits, bad.to(DEV), 1.0, loss, ws)
        with pytest.raises(EmageKernelError):
            ops.loss_check(ws)


@pytest.mark.parametrize("m", fc.COLSUM_M)
def test_col_sum(m):
    fc.check_col_sum(ops, m)


def test_transpose():
    fc.check_transpose(ops)


@pytest.mark.parametrize("b,t,c,res,swap", fc.MUL_ADD_CASES)
def test_mul_add(b, t, c, res, swap):
    fc.check_mul_add(ops, b, t, c, res, swap)


@pytest.mark.parametrize("start,wd", fc.ADAM_CASES)
@pytest.mark.parametrize("entry", ["step", "step_dev", "multi"])
def test_adam(entry, start, wd):
    fc.check_adam(ops, entry, start, wd)


def test_adam_skip():
    fc.check_adam_skip(ops)


@pytest.mark.parametrize("c", fc.ARGMAX_C)
def test_argmax_logsoftmax(c):
    fc.check_argmax(ops, c)


def test_rotations():
    fc.check_aa_to_rot6d(ops)
    fc.check_rot6d_to_aa(ops)


@pytest.mark.parametrize("m", [1, 5])
def test_merge_parts(m):
    fc.check_merge_parts(ops, m)


@pytest.mark.parametrize("b,t,col0,init", fc.VEL_CASES)
def test_velocity_to_position(b, t, col0, init):
    fc.check_velocity(ops, b, t, col0, init)
