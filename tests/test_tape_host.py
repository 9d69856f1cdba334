"""Host logic of the two owners in pantomatrix_amd/tape.py on the CPU stand-ins of the kernels: `ParamGrads.discard()`, and what the three
callers of a backward — `TrainForward.backward_from`, `training_vq._TokenizerFn.backward`, `Trainer.step` — leave behind when a tape node
raises mid-walk: the original exception, an empty queue (adds AND finalize entries), the caller's accumulators back in place, and a next
backward that is the one of a fresh forward object."""
import contextlib

import pytest
import torch

import common
import fake_ops
import train_common as tc
import vq_train_common as vc
from pantomatrix_amd import ops, tape, training, training_vq
from test_vq_train_host import _installed as vq_installed


class Boom(Exception):
    pass


@contextlib.contextmanager
def deferring():
    """Inside `fake_ops.installed()`: a `col_sum` stand-in that HONOURS `defer` (fake_ops applies the sum at once) — the float64 partial is
    queued in the `ops.FinalizeQueue`, and the queue's multi-finalize launch is restated on the CPU."""
    def col_sum(x, y=None, out=None, accumulate=False, defer=None):
        if defer is None or out is None:
            return fake_ops.col_sum(x, y, out, accumulate)
        fake_ops.CALLS.append("col_sum")
        defer.add((x.double() * (y.double() if y is not None else 1.0)).sum(0), 1, x.shape[1], out, accumulate)
        return out

    def finalize_multi(outs, partials, desc):
        for k, (o, p) in enumerate(zip(outs, partials)):
            o.copy_(o + p.float() if desc[3 * k + 2] else p.float())

    saved = ops.col_sum, ops._col_sum_finalize_multi
    ops.col_sum, ops._col_sum_finalize_multi = col_sum, finalize_multi
    try:
        yield
    finally:
        ops.col_sum, ops._col_sum_finalize_multi = saved


def dying_node(fwd, boom, seen, weight, bias):
    """A tape node that queues one add and one finalize entry through the forward's own spellings, then dies."""
    def node():
        p = fwd._param(weight)
        fwd._param_grad(weight, slice(None), torch.ones_like(p, dtype=torch.float32))
        fwd.grads.add_colsum(bias, slice(None), torch.ones(3, fwd._param(bias).shape[0]))
        seen.append(fwd.grads.pending())
        raise boom
    return node


def same_grads(got, want):
    assert set(got) == set(want) and len(want) > 0
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_discard_drops_what_is_queued_and_nothing_else():
    """Overlapping and disjoint contributions, adds and column sums: after `discard()` the accumulators hold exactly what was flushed
    before it — the overlap flushed the first batch — and a later flush adds nothing."""
    params = {"w": torch.zeros(8, 4), "b": torch.zeros(8)}
    pg = tape.ParamGrads(params.__getitem__, lambda: 0)
    ref = {k: torch.zeros_like(v) for k, v in params.items()}
    with fake_ops.installed(), deferring():
        first = [("w", slice(0, 4), torch.full((4, 4), 1.0)), ("w", slice(4, 8), torch.full((4, 4), 2.0)), ("b", slice(None), torch.arange(8.0))]
        for name, rows, g in first:
            pg.add(name, rows, g)
            ref[name][rows] += g
        pg.add_colsum("b", slice(0, 4), torch.ones(5, 4))        # direct accumulation into rows with a queued add: the queue goes first
        assert pg.pending() == (0, 1)                            # ... and the column sum's finalize waits
        pg.add("w", slice(2, 6), torch.full((4, 4), 4.0))        # an add (would overlap what was flushed): queued
        pg.add("w", slice(6, 8), torch.full((2, 4), 8.0))        # disjoint from it: the same batch
        assert pg.pending() == (2, 1)
        pg.discard()
        assert pg.pending() == (0, 0)
        for k in ref:
            assert torch.equal(pg.acc[k], ref[k]), k
        assert pg.current() is pg.acc                            # reading flushes: there is nothing left to apply
        for k in ref:
            assert torch.equal(pg.acc[k], ref[k]), k
        pg.add_colsum("b", slice(0, 4), torch.ones(5, 4))        # the owner still works: a flushed column sum arrives
        ref["b"][0:4] += 5.0
        assert torch.equal(pg.current()["b"], ref["b"])


def test_alone_restores_the_callers_accumulators():
    pg = tape.ParamGrads({"w": torch.zeros(2, 2)}.__getitem__, lambda: 0)
    mine = {}
    pg.start(mine)
    pg.add("w", slice(None), torch.ones(2, 2))
    with pg.alone() as own:
        assert float(mine["w"].sum()) == 4.0                     # what was queued for the caller's dict went there first
        pg.add("w", slice(None), torch.full((2, 2), 3.0))
    assert float(own["w"].sum()) == 12.0 and pg.acc is mine and float(mine["w"].sum()) == 4.0
    with pytest.raises(Boom):
        with pg.alone():
            pg.add("w", slice(None), torch.ones(2, 2))
            raise Boom()
    assert pg.pending() == (0, 0) and pg.acc is mine and float(mine["w"].sum()) == 4.0


def test_backward_from_that_dies_mid_walk_leaves_nothing_queued():
    (audio, spk, motion, mask), ref, masks, _ = tc.oracle_forward(seed=7)
    model, _ = common.product_models(precision="fp32")
    gouts = {k: torch.randn(v.shape, generator=torch.Generator().manual_seed(1)) for k, v in ref.items()}

    def run(fwd, node=None):
        fwd(audio, spk, motion, mask, masks, tape=True)
        t, out2d, fwd.tape = fwd.tape, fwd._out2d, None
        if node is not None:
            t.nodes[len(t.nodes) // 2] = node
        return fwd.backward_from(t, out2d, gouts)

    fwd, boom, seen = training.TrainForward(model), Boom("node"), []
    mine = {"kept": torch.ones(1)}
    with fake_ops.installed(), deferring(), torch.no_grad():
        fwd.param_grads = mine
        with pytest.raises(Boom) as exc:
            run(fwd, dying_node(fwd, boom, seen, "face_out_proj.weight", "face_out_proj.bias"))
        assert exc.value is boom
        assert seen and seen[0][0] >= 1 and seen[0][1] >= 1      # the node did die with adds and finalize entries queued
        assert fwd.grads.pending() == (0, 0)
        assert fwd.param_grads is mine and set(mine) == {"kept"} and fwd.tape is None
        got = run(fwd)
        want = run(training.TrainForward(model))
    same_grads(got, want)
    assert fwd.param_grads is mine and set(mine) == {"kept"}


def test_tokenizer_backward_that_dies_mid_walk_leaves_nothing_queued():
    x = vc.case_input("vq2")

    def grads_of(m, node_for=None):
        m.zero_grad()
        out = m(x)
        loss = torch.nn.functional.mse_loss(out["rec_pose"], x) + out["embedding_loss"]
        if node_for is not None:
            t = out["rec_pose"].grad_fn.saved[0]
            t.nodes[len(t.nodes) // 2] = node_for
        loss.backward()
        return {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}

    m = vc.product_model("vq2", "fp32")
    boom, seen, mine = Boom("node"), [], {"kept": torch.ones(1)}
    with vq_installed(), deferring():
        m.unfreeze().train()
        with torch.no_grad():
            m(x[:1, :8])                                          # creates the model's forward object
        fwd = m.__dict__["_train_fwd"]
        assert isinstance(fwd, training_vq.TokenizerForward) and not isinstance(fwd, training.TrainForward)
        fwd.param_grads = mine
        with pytest.raises(Boom) as exc:
            grads_of(m, dying_node(fwd, boom, seen, "decoder.main.0.model.0.weight", "decoder.main.0.model.0.bias"))
        assert exc.value is boom
        assert seen and seen[0][0] >= 1 and seen[0][1] >= 1
        assert fwd.grads.pending() == (0, 0)
        assert fwd.param_grads is mine and set(mine) == {"kept"} and fwd.tape is None
        got = grads_of(m)
        fresh = vc.product_model("vq2", "fp32")
        fresh.unfreeze().train()
        want = grads_of(fresh)
    same_grads(got, want)
    assert fwd.param_grads is mine and set(mine) == {"kept"}


def test_trainer_step_that_dies_mid_backward_leaves_nothing_queued(monkeypatch):
    from test_train_oracle import train_batch
    batch = train_batch(bs=2)
    random_mask = (torch.rand(2, 64, 337, generator=torch.Generator().manual_seed(3)) < 0.5).float()
    model, vq = common.product_models(precision="fp32")
    trainer = training.Trainer(model, vq, seed=7)
    fwd, boom, seen, calls = trainer.fwd, Boom("node"), [], []
    real = training.TrainForward.backward

    def backward(self, index_gt, latent_gt, progress=None):
        calls.append(self)
        if self is fwd and len(calls) == 2:                      # the step's SECOND backward: the buckets already hold the first one's gradients
            self.tape.nodes[len(self.tape.nodes) // 2] = dying_node(self, boom, seen, "face_out_proj.weight", "face_out_proj.bias")
        return real(self, index_gt, latent_gt, progress)

    monkeypatch.setattr(training.TrainForward, "backward", backward)
    with fake_ops.installed(), deferring(), torch.no_grad():
        with pytest.raises(Boom) as exc:
            trainer.step(batch, random_mask=random_mask)
        assert exc.value is boom
        assert seen and seen[0][0] >= 1 and seen[0][1] >= 1
        assert fwd.grads.pending() == (0, 0)
        assert all(float(b.abs().max()) == 0.0 for b in trainer.buckets.flat) and trainer.steps_done == 0
        got, want = {}, {}
        l_got = trainer.step(batch, random_mask=random_mask, grad_hook=lambda g: got.update({k: v.clone() for k, v in g.items()}))
        model2, _ = common.product_models(precision="fp32")
        l_want = training.Trainer(model2, vq, seed=7).step(batch, random_mask=random_mask, grad_hook=lambda g: want.update({k: v.clone() for k, v in g.items()}))
    assert l_got == l_want
    same_grads(got, want)
    p, q = model._flat_params(), model2._flat_params()
    assert all(torch.equal(p[k], q[k]) for k in q)
