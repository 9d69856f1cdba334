"""The case table of tests/forward_cases.py run through the fp32 stand-ins of tests/fake_ops.py on the CPU: a correct fp32 implementation
(torch's own layer_norm / log_softmax / fp32 arithmetic, the fp32 oracle rotations) passes every tolerance the GPU test applies, every wrong
reference is rejected, and the input conditions hold (the argmax top-2 gap of every row).  No GPU."""
import pytest
import torch

import fake_ops as F
import forward_cases as fc


@pytest.mark.parametrize("c", fc.LN_C)
@pytest.mark.parametrize("name", list(fc.LN_DTYPES))
def test_layernorm(name, c):
    fc.check_layernorm(F, name, c)


@pytest.mark.parametrize("m", fc.BN_M)
def test_bn_stats(m):
    fc.check_bn_stats(F, m)


@pytest.mark.parametrize("m,c,mode,slope", fc.BN_APPLY_CASES)
def test_bn_apply(m, c, mode, slope):
    fc.check_bn_apply(F, m, c, mode, slope)


def test_bn_apply_torch_batch_norm():
    """torch's own fp32 batch_norm on the CPU passes the bn_apply tolerance as well."""
    class T:
        @staticmethod
        def bn_apply(x, stats, gamma, beta, out, *, slope=1.0, sc=None, sc_bn=None, eps=1e-5):
            bn = lambda v, mu, var, g, b: torch.nn.functional.batch_norm(v, mu, var, g, b, False, 0.0, eps)
            v = bn(x, *stats, gamma, beta)
            if sc is not None:
                v = v + (bn(sc, *sc_bn) if sc_bn is not None else sc)
            out.copy_(torch.nn.functional.leaky_relu(v, slope))
    for case in fc.BN_APPLY_CASES[:-1]:
        fc.check_bn_apply(T, *case)


@pytest.mark.parametrize("m,c", fc.MSE_SHAPES)
def test_mse_loss(m, c):
    fc.check_mse_loss(F, m, c)


@pytest.mark.parametrize("m,k", fc.NLL_SHAPES)
def test_nll_loss(m, k):
    fc.check_nll_loss(F, m, k)


@pytest.mark.parametrize("m", fc.COLSUM_M)
def test_col_sum(m):
    fc.check_col_sum(F, m)


def test_transpose():
    fc.check_transpose(F)


@pytest.mark.parametrize("b,t,c,res,swap", fc.MUL_ADD_CASES)
def test_mul_add(b, t, c, res, swap):
    fc.check_mul_add(F, b, t, c, res, swap)


@pytest.mark.parametrize("start,wd", fc.ADAM_CASES)
@pytest.mark.parametrize("entry", ["step", "multi"])
def test_adam(entry, start, wd):
    fc.check_adam(F, entry, start, wd)


class TorchAdam:
    """torch's own fp32 optimizer on the CPU behind the `adam_step` signature."""

    @staticmethod
    def adam_step(param, grad, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps, weight_decay):
        w = param.clone().requires_grad_()
        opt = torch.optim.Adam([w], lr=lr, betas=(beta1, beta2), eps=eps, weight_decay=weight_decay)
        opt.state[w] = dict(step=torch.tensor(float(int(step) - 1)), exp_avg=exp_avg, exp_avg_sq=exp_avg_sq)       # updated in place
        w.grad = grad.clone()
        opt.step()
        param.copy_(w.detach())


@pytest.mark.parametrize("start,wd", fc.ADAM_CASES)
def test_adam_torch_fp32(start, wd):
    """torch.optim.Adam in fp32 passes the same tolerances."""
    fc.check_adam(TorchAdam, "step", start, wd)


def test_adam_skip():
    fc.check_adam_skip(F)


@pytest.mark.parametrize("c", fc.ARGMAX_C)
def test_argmax_logsoftmax(c):
    """Also the input condition: every row's float64 top-2 gap is exactly 0 or above 1e-3 of the row's scale (asserted inside for every
    row of every case, and here that the condition can fail at all)."""
    fc.check_argmax(F, c)
    assert not fc.argmax_gap_ok(torch.tensor([[1.0, 1.0005, 0.0]]))
    assert fc.argmax_gap_ok(torch.tensor([[1.0, 1.0, 0.0], [1.0, 1.002, 0.0]]))


def test_rotations():
    """The fp32 oracle passes aa -> 6-D at the derived tolerance; in 6-D -> aa it is the yardstick itself (the kernel may be 4 x its
    per-class error), so here it passes by construction and the table shows the class errors."""
    fc.check_aa_to_rot6d(F)
    table = fc.check_rot6d_to_aa(F)
    assert all(err <= max(4 * orc_err, fc.ROT_FLOOR) for _, orc_err, err in table)


@pytest.mark.parametrize("m", [1, 5])
def test_merge_parts(m):
    fc.check_merge_parts(F, m)


@pytest.mark.parametrize("b,t,col0,init", fc.VEL_CASES)
def test_velocity_to_position(b, t, col0, init):
    fc.check_velocity(F, b, t, col0, init)
