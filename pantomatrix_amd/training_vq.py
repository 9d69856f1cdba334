"""The motion tokenizers in TRAIN mode on the MI355X kernels: `EmageVQVAEConv` (encoder -> Quantizer -> decoder, M:34-46) and
`EmageVAEConv` (encoder -> decoder, M:19-32) of the reference's models/emage_audio/modeling_emage_audio.py, differentiable.

The conv stacks are `tape.TapeForward`'s tape-aware `_conv3` (the same Conv1d(k=3) + LeakyReLU(0.2) + ResBlock layers the EMAGE
training forward runs for its motion pre-encoder, with the same backward contractions); the quantiser (P:144-156) is
`emage_vq_argmin_f32` (the one kernel pinned to the reference's association and tie rule) followed by `emage_vq_quantize_train`
(codebook rows, histogram, embedding_loss and perplexity as device scalars), and on the way back `emage_vq_quantize_backward`
(straight-through + commitment gradient of the encoder output, the codebook gradient in a fixed summation order).

Three ways in, all opt-in (`model.unfreeze()`; a fresh tokenizer is frozen and its `.train()` raises, as before):
  * the class API: `m.unfreeze().train(); out = m(x); loss.backward(); torch.optim.Adam(m.parameters()).step()` (`train_forward`);
  * `TokenizerForward(model)(x, tape=True)` + `backward(...)`: the launches without torch autograd;
  * `TokenizerTrainer(model).step(x)`: forward, mse(rec_pose, x) (+ embedding_loss), backward, one multi-tensor Adam launch.
f16x3 (float32 storage, split-fp16 contractions) and fp32; bf16 raises, as `TrainForward` does.  No CPU fallback."""
from __future__ import annotations

import torch

from . import ops
from .modeling_emage_audio import _Ctx, _rup
from .tape import TapeForward, _check_max_norm, _param_grad_norms, clip_and_adam

CODEBOOK = "quantizer.embedding.weight"


class TokenizerForward(TapeForward):
    """Callable train-mode forward of an `EmageVQVAEConv` / `EmageVAEConv` with a tape; `backward()` runs it from output gradients."""

    def __init__(self, model):
        super().__init__(model)
        self.quantized = CODEBOOK in model._spec
        self._zq = self._rec = self._scalars = None
        self._g_loss = None

    def __call__(self, inputs, tape=False):
        """inputs (B, T, vae_test_dim) -> dict(rec_pose (B, T, dim)) and, for the VQ class, poses_feat (B, T, vae_length) + the device
        scalars embedding_loss / perplexity (0-dim fp32 views).  tape=True keeps what `backward()` needs."""
        model, c = self.model, self.model.config
        cx = _Ctx(model._engine(h2=False, train_only=True))
        dev = cx.dev
        self._begin_forward(cx, tape)
        b, t, d = inputs.shape
        length = c.vae_length
        x = ops.cast_pad(cx.dt, inputs.reshape(b * t, d).to(device=dev, dtype=torch.float32).contiguous(), _rup(d))
        pre = self._conv_encoder(cx, "encoder", x, t, b, d, c.vae_layer, need_dx=False)              # (M, rup64(length)) fp32
        out = {}
        if self.quantized:
            z, zin = self._quantize(cx, pre, length)
            out["poses_feat"] = z.view(b, t, length)
            out["embedding_loss"], out["perplexity"] = self._scalars[0], self._scalars[1]
        else:
            zin = pre
        rec = self._conv_decoder(cx, "decoder", zin, t, b, length, c.vae_layer)                        # (M, rup64(dim))
        self._rec = rec
        out["rec_pose"] = (rec if rec.shape[1] == d else rec[:, :d]).reshape(b, t, d)
        return out

    def _quantize(self, cx, pre, length):
        """Quantizer.forward (P:144-156): -> (z_q (M, length) fp32, the decoder's operand (M, rup64(length)))."""
        beta = float(self.model.config.vae_quantizer_lambda)
        codebook = cx.pk.w["codebook"]
        z = pre if pre.shape[1] == length else pre[:, :length]
        idx = ops.vq_argmin(z, codebook)
        padded = _rup(length) != length
        zq, img, _hist, self._scalars = ops.vq_quantize_train(z, codebook, idx, beta, image_dtype=cx.dt if padded else None, n_store=_rup(length))
        zin = img if padded else zq                       # float32 storage: the rows themselves are the operand when no padding is needed
        self._zq = zq
        if self.tape is not None:
            def bw():
                g = self.tape.get(zq)
                if zin is not zq:                         # the decoder's gradient arrived at the padded image
                    gi = self.tape.get(zin)
                    if gi is not None:
                        gi = gi[:, :length]
                        g = gi.contiguous() if g is None else g + gi
                if g is None and self._g_loss is None:
                    return
                g_loss = self._g_loss if self._g_loss is not None else torch.zeros(1, dtype=torch.float32, device=cx.dev)
                dz, de = ops.vq_quantize_backward(z, codebook, idx, g, g_loss, beta)
                self.tape.add(pre, dz, cols=length)
                self._param_grad(CODEBOOK, slice(None), de)
            self.tape.node(bw)
        return zq, zin

    def backward(self, g_rec=None, g_feat=None, g_loss=None):
        """Gradients of the LAST forward (tape=True) from the gradients of its outputs — g_rec (B, T, dim), g_feat (B, T, vae_length), g_loss
        a one-element DEVICE tensor (d loss / d embedding_loss) — accumulated into `param_grads` (name -> fp32 tensor)."""
        if self.tape is None:
            raise RuntimeError("backward() needs the forward to be run with tape=True")
        tape, rec = self.tape, self._rec
        if g_rec is not None:
            g = g_rec.reshape(rec.shape[0], -1).to(torch.float32)
            if g.shape[1] != rec.shape[1]:
                g = torch.nn.functional.pad(g, (0, rec.shape[1] - g.shape[1]))
            tape.add(rec, g.contiguous())
        if g_feat is not None and self.quantized:
            tape.add(self._zq, g_feat.reshape(self._zq.shape).to(torch.float32).contiguous())
        self._g_loss = None if g_loss is None else g_loss.reshape(1).to(torch.float32)
        try:
            tape.run()
            self.flush_param_grads()
        finally:
            self._g_loss, self.tape = None, None
        return self.param_grads


# ======================================================================================
# the autograd bridge: `m.unfreeze().train(); out = m(x); loss.backward()`
# ======================================================================================
class _TokenizerFn(torch.autograd.Function):
    """One train-mode forward of a tokenizer as ONE autograd node (cf. `training._TrainFn`): the parameters are inputs of the node, so
    `.grad` accumulation and optimisers behave as for the reference module.  perplexity carries no gradient (it has none in the reference)."""

    @staticmethod
    def forward(ctx, fwd, names, inputs, *params):
        with torch.no_grad():
            out = fwd(inputs, tape=True)
        ctx.fwd, ctx.names = fwd, names
        ctx.saved = (fwd.tape, fwd._rec, fwd._zq)
        fwd.tape = None
        if not fwd.quantized:
            return (out["rec_pose"],)
        perplexity = out["perplexity"].clone()
        ctx.mark_non_differentiable(perplexity)
        return out["rec_pose"], out["poses_feat"], out["embedding_loss"].clone(), perplexity

    @staticmethod
    def backward(ctx, g_rec, g_feat=None, g_loss=None, _g_perplexity=None):
        fwd = ctx.fwd
        fwd.tape, fwd._rec, fwd._zq = ctx.saved
        ctx.saved = None
        with fwd.grads.alone():                           # the gradients of this node alone; the caller's accumulators are back behind it
            grads = fwd.backward(g_rec, g_feat, g_loss)
            fwd.flush_range_checks(new_step=True)
            if fwd.range_flag is not None and int(fwd.range_flag) != 0:      # a weight left the band its cached operand scale was chosen for
                fwd.reset_scales()
        return (None, None, None) + tuple(grads.get(n) for n in ctx.names)


def train_forward(model, inputs):
    """`EmageVQVAEConv.forward` / `EmageVAEConv.forward` in TRAINING mode (what `model(x)` runs after `model.unfreeze().train()`)."""
    fwd = model.__dict__.get("_train_fwd")
    if fwd is None:
        fwd = model.__dict__["_train_fwd"] = TokenizerForward(model)
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    outs = _TokenizerFn.apply(fwd, [n for n, _p in named], inputs, *[p for _n, p in named])
    keys = ("rec_pose", "poses_feat", "embedding_loss", "perplexity") if fwd.quantized else ("rec_pose",)
    out = dict(zip(keys, outs))
    return {k: out[k] for k in ("poses_feat", "embedding_loss", "perplexity", "rec_pose") if k in out}


# ======================================================================================
# the minimal objective on the device: mse(rec_pose, x) (+ embedding_loss), Adam
# ======================================================================================
class TokenizerTrainer:
    """`step(x)`: train-mode forward, `emage_mse_loss` of rec_pose against the input (+ embedding_loss for the VQ class), backward,
    `emage_adam_multi` over every parameter with the step count on the device.  No torch autograd; the only host read-back is the
    returned losses.  Every sum of the step has a fixed order: two steps from the same state and input give the same bits.
    max_grad_norm / track_grad_norm: as for `training.Trainer` — `ops.grad_norm` over the Adam table in front of Adam, the clip
    coefficient as Adam's device-side gradient factor, "grad_norm" in the returned dict, `param_grad_norms()`."""

    def __init__(self, model, lr=1.5e-4, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, track_grad_norm=False):
        model.unfreeze()
        self.model, self.fwd = model, TokenizerForward(model)
        self.lr, self.betas, self.eps = lr, betas, eps
        dev = model.device
        params = model._flat_params()
        self.names = [n for n, p in model.named_parameters() if p.requires_grad]
        self.grads = {n: torch.zeros_like(params[n], dtype=torch.float32) for n in self.names}
        self.state = {n: dict(exp_avg=torch.zeros_like(params[n]), exp_avg_sq=torch.zeros_like(params[n])) for n in self.names}
        self._adam = ops.AdamTable([(params[n], self.grads[n], self.state[n]["exp_avg"], self.state[n]["exp_avg_sq"]) for n in self.names], dev)
        self._params = [params[n] for n in self.names]
        self.step_counter = torch.zeros(1, dtype=torch.int32, device=dev)
        self._one = torch.ones(1, dtype=torch.float32, device=dev)
        self.health = torch.zeros(1, dtype=torch.int32, device=dev)       # non-finite gradient words of the last step (Adam's skip word)
        self.steps_done = 0
        self.max_grad_norm, self.track_grad_norm = _check_max_norm(max_grad_norm), bool(track_grad_norm)
        self._grad_norm = None

    def param_grad_norms(self):
        """{parameter name: 2-norm of its gradient} of the last step — one device-to-host copy of the float64 sums of squares."""
        return _param_grad_norms(self._grad_norm, self.names, 1.0)

    def step(self, x, grad_hook=None):
        """One optimisation step on x (B, T, vae_test_dim) -> dict of the losses as Python floats ("rec", "all"; the VQ class adds
        "embedding_loss" and "perplexity").  `grad_hook(grads)` runs between backward and the update, as `Trainer.step`'s does."""
        fwd = self.fwd
        dev = self.model.device
        fwd.grad_views, fwd.param_grads = self.grads, {}
        b, t, d = x.shape
        x2d = x.reshape(b * t, d).to(device=dev, dtype=torch.float32).contiguous()
        out = fwd(x2d.view(b, t, d), tape=True)
        rec_full = fwd._rec
        rec2d = rec_full if rec_full.shape[1] == d else rec_full[:, :d]
        ws = ops.loss_workspace(dev)
        rec_loss = torch.zeros(1, dtype=torch.float64, device=dev)
        ops.mse_loss(rec2d, x2d, 1.0, rec_loss, ws)
        g = torch.zeros_like(rec_full)                          # the padding columns of the last layer carry no gradient
        ops._mse_loss_grad(rec2d, x2d, 1.0, g if g.shape[1] == d else g[:, :d])
        fwd.tape.add(rec_full, g)
        fwd.backward(g_loss=self._one if fwd.quantized else None)
        if grad_hook is not None:
            grad_hook(self.grads)
        fwd.flush_range_checks(new_step=True)
        # inf / NaN among the gradients (an fp16 plane of the split-fp16 backward overflowed) -> Adam's skip word: such a step never reaches the weights
        self.health.zero_()
        ops.count_nonfinite_multi(list(self.grads.values()), self.health)
        self.step_counter.add_(1)
        norm = clip_and_adam(self._adam, self.step_counter, self.lr, self.betas, self.eps, 0.0, self.health,
                             max_norm=_check_max_norm(self.max_grad_norm), track=self.track_grad_norm)
        tracking = norm is not None
        if tracking:
            self._grad_norm = norm
        self.step_counter.sub_((self.health > 0).to(torch.int32))       # a skipped step does not count
        self.model.bump_versions(self._params)                  # updated through raw pointers: the next `_engine()` re-packs
        res = {"rec": float(rec_loss)}
        grad_norm = float(self._grad_norm.norm) if tracking else None
        bad = int(self.health[0])
        if fwd.range_flag is not None and int(fwd.range_flag) != 0:      # a weight left the band its cached operand scale was chosen for
            fwd.reset_scales()
        if bad:
            raise FloatingPointError(f"tokenizer training step {self.steps_done + 1}: {bad} non-finite gradient words — the update was skipped on the "
                                     f"device (precision {self.model.precision!r}, grad_scale {fwd.grad_scale:g}); lower `fwd.grad_scale` or train in fp32")
        self.steps_done += 1
        res["all"] = res["rec"]
        if fwd.quantized:
            res["embedding_loss"], res["perplexity"] = float(out["embedding_loss"]), float(out["perplexity"])
            res["all"] += res["embedding_loss"]
        if grad_norm is not None:
            res["grad_norm"] = grad_norm
        return res
