"""EmageAudioModel.forward in TRAIN mode on the MI355X kernels — the forward half of the EMAGE training step
(/root/reference/train_emage_audio.py:130-204 drives three such forwards per step).

What differs from the inference forward (`modeling_emage_audio.EmageAudioModel.forward`), all of it behaviour of torch
modules inside /root/reference/models/emage_audio/modeling_emage_audio.py (M:) and processing_emage_audio.py (P:):

  * the two WavEncoders (P:262-314) run nn.BatchNorm1d with BATCH statistics: the convolutions are launched with their raw
    weights (no BatchNorm fold), `emage_bn_stats` reduces each conv output over all clips and positions (float64 sums) and
    updates the running statistics the way torch does, `emage_bn_apply` normalises and applies what follows inside
    BasicBlock.forward (P:283-294: LeakyReLU; the shortcut, itself batch-normalised in the downsample blocks);
  * dropout (p = 0.1) at every site torch has one — PeriodicPositionalEncoding (P:341-343), and inside
    nn.TransformerEncoderLayer / nn.TransformerDecoderLayer (M:238-262): on the attention probabilities
    (`emage_attention_dropout`), on each sub-layer output before the residual add, inside the FFN (`emage_mul_add`).

Randomness is an INPUT: `dropout_masks` is the list of mask tensors (values bernoulli / (1 - p)) in the order the reference
draws them and in the logical shapes its modules see — (B, T, d) for the positional encodings, (B, H, Tq, Tk) for attention
probabilities, (T, B, C) for the layers' dropouts (its layers are batch_first=False).  The parity tests take the masks from
the CPU oracle's replay of the reference's generator draws (oracle/emage_train_oracle.py), so outputs, BatchNorm buffers
and losses can be compared number for number; a training loop would fill them from a device generator.

No CPU fallback: every arithmetic step is a launch into libemage_hip.so.  Backward, Adam and the gradient exchange
(pantomatrix_amd/dist.py has the bucket plan) are the next pieces of this row.
"""
from __future__ import annotations

import contextlib

import torch

from . import ops, spec
from ._lib import F32, H2
from .modeling_emage_audio import OUT_KEYS, _Ctx, _WAV_TAPS, _rup
from .tape import DROPOUT_P, TapeForward, _Masks, _Tape, _Token, _capturing, _check_max_norm, _param_grad_norms, clip_and_adam      # noqa: F401 (re-exports)

BN_MOMENTUM = 0.1          # nn.BatchNorm1d default


def dropout_mask_count():
    """Masks one train-mode forward consumes: 3 positional encodings, 15 decoder layers x 6, 1 encoder layer x 4."""
    return 3 + 6 * (spec.N_FACE_LAYERS + spec.N_CROSS_LAYERS + 3) + 4


_ZERO_LONG = torch.zeros((), dtype=torch.long)           # stands for a missing `num_batches_tracked` buffer


class StepShare:
    """What the forwards of ONE optimisation step share.  The reference runs both WavEncoders in each of the three forwards of a step
    (T:156-172) on the SAME audio with the SAME weights: the same features and the same batch statistics three times, and three backward
    passes through them whose parameter gradients are summed.  Here the first forward's encoder pass is kept — features, BatchNorm
    statistics (later forwards replay the running-buffer updates from them), and its own tape — and the encoders are differentiated ONCE,
    behind the third backward, from the SUM of the three feature gradients (the backward is linear in them): 1/3 of the WavEncoder work of a
    step, and 1/3 of its SyncBatchNorm exchanges."""

    def __init__(self):
        self.feats, self.tape, self.bn_log = None, None, []


class TrainForward(TapeForward):
    """Callable train-mode forward of an `EmageAudioModel` (f16x3 or fp32 precision), with `backward()` for the part of the
    network behind the convolutional front ends.  The tape-aware layer wrappers, the parameter-gradient accumulation and the backward
    operand scales are `tape.TapeForward`'s."""

    def __init__(self, model, sync_bn=False, group=None):
        """sync_bn: BatchNorm statistics (forward) and their gradient sums (backward) are taken over all ranks of `group`, the
        behaviour of nn.SyncBatchNorm the reference converts its model to (train_emage_audio.py:248); torch.distributed must be
        initialised."""
        super().__init__(model)
        self.sync_bn, self.group, self._bn_count = sync_bn, group, {}
        self._clips = {}                # local clip count -> clips of all ranks (sync_bn: exchanged at the first BatchNorm of EVERY eager forward, see `_clip_total`)
        self._bn_log = None             # list collecting (name, mean, var, rows) of a WavEncoder pass that later forwards of the step replay
        self.lazy_masks = True          # device-drawn (T, B, d) dropout masks live as Philox keys: drawn inside `mul_add`, forward and backward (-0.9 GB per forward)
        self._shared, self.last_run_nodes = None, 0

    # ---- packing of what the inference pack does not hold: un-folded WavEncoder convolutions ----------------------------
    def _train_pack(self, pk):
        if "train.wav_in" in pk.w:
            return
        m = self.model
        w0, b0 = [], []
        for enc in ("audio_encoder_face", "audio_encoder_body"):
            for i, (cin, cout, stride, pad, ds) in enumerate(m._wav_blocks()):
                base = f"{enc}.feat_extractor.{i}"
                if i == 0:
                    for conv in (base + ".conv1", base + ".downsample.0"):
                        w, b = pk.folded(conv, None)
                        w0.append(w.reshape(cout, _WAV_TAPS))
                        b0.append(b)
                else:
                    pk.conv(base + ".conv1.raw", base + ".conv1", extra=(base + ".downsample.0", None) if ds else None)
                pk.conv(base + ".conv2.raw", base + ".conv2")
                for bn in ("bn1", "bn2") + (("downsample.1",) if ds else ()):
                    pk.w[f"{base}.{bn}.affine"] = (pk.f32(f"{base}.{bn}.weight"), pk.f32(f"{base}.{bn}.bias"))
        pk.w["train.wav_in"] = dict(w=torch.cat(w0, 0).float().contiguous(), b=torch.cat(b0).float().contiguous())
        pk.w["train.ones"] = torch.ones(pk.w["train.wav_in"]["w"].shape[0], dtype=torch.float32, device=pk.device)
        pk.finish_range_check()

    # ---- BatchNorm bookkeeping ----------------------------------------------------------------------------------------------
    def _global_rows(self, rows, b):
        """Rows of a BatchNorm input over the GLOBAL batch (nn.SyncBatchNorm's count): every rank runs the same sequence lengths, so it is
        rows / b x (clips of all ranks) — host arithmetic on the clip total exchanged ONCE per forward / step (`_clip_total`), no read-back
        of a device count per BatchNorm."""
        return rows // b * self._clip_total(b)

    def begin_step(self):
        """Start of an optimisation step (`Trainer._device_step`): outside a graph capture the global clip count of SyncBatchNorm is
        forgotten, so the step's first BatchNorm exchanges it afresh (`_clip_total`)."""
        if self.sync_bn and not _capturing(self.model.device):
            self._clips.clear()

    @contextlib.contextmanager
    def step(self):
        """One optimisation step: `begin_step`, then the step's forwards and backwards inside.  The parameters move at the END of the step,
        so ONE set of transposed weight images, built afresh, serves all of them and is dropped behind the step; a step that dies takes what
        it had queued for the gradient accumulators with it (its float64 partials would otherwise land in the NEXT step's buckets)."""
        self.begin_step()
        with self.scales.keep_images():
            try:
                yield self
            except BaseException:
                self.grads.discard()
                raise

    def _clip_total(self, b):
        """Clips of all ranks for a local batch of b clips (sync_bn).  Exchanged — one small all-reduce with a host read-back — at the first
        BatchNorm of EVERY eager step (`begin_step`; of every eager forward outside a step: `__call__`) — with the shared encoder pass that is
        once per step —, on every rank at the same point of the launch sequence, so the collectives always pair and a rank whose neighbour changed
        its batch size never divides by a stale count.  Inside a graph capture the host cannot read a device count: the
        value of the warm-up step is used, and `Trainer.capture` documents the contract that goes with it — every rank replays the batch
        sizes it captured (a changed batch needs a re-capture on ALL ranks, as the collectives inside the graphs must pair anyway)."""
        if not self.sync_bn:
            return b
        hit = self._clips.get(b)
        if hit is None:
            if _capturing(self.model.device):
                raise RuntimeError("TrainForward: the global clip count of a SyncBatchNorm step must be known before a graph capture "
                                   "(run one eager step with the same batch size first: Trainer.capture does)")
            from . import dist as pdist
            hit = self._clips[b] = pdist.total_over_group(b, device=self.model.device, group=self.group)
        return hit

    def _bn_many(self, cx, items, b, new_stats):
        """Batch statistics of several INDEPENDENT BatchNorms: items = [(name, conv output x (M, C))] -> [(mean, biased var)]; the running
        buffers advance in `new_stats`.  sync_bn (nn.SyncBatchNorm, T:248): the local (mean, variance, rows) of ALL items travel in ONE
        all-gather and are merged count-weighted in float64 (`dist.merge_batch_stats_many`) — the two encoders' bn1 of a block, or their
        bn2 + shortcut BatchNorms, are one collective instead of two / four."""
        params = self._params()
        out = []
        if self.sync_bn:
            from . import dist as pdist
            local = [ops.bn_stats(x, None, None, BN_MOMENTUM) for _name, x in items]
            merged = pdist.merge_batch_stats_many([(mean, var, x.shape[0]) for (mean, var), (_name, x) in zip(local, items)], group=self.group)
        # fresh copies of the running buffers (updated in place below) and the advanced batch counters of ALL items: three multi-tensor launches
        src = lambda nm, sfx: new_stats.get(nm + sfx, params[nm + sfx]).detach()
        rms = torch._foreach_mul([src(name, ".running_mean").to(cx.dev, torch.float32) for name, _x in items], 1.0)
        rvs = torch._foreach_mul([src(name, ".running_var").to(cx.dev, torch.float32) for name, _x in items], 1.0)
        nbts = torch._foreach_add([new_stats.get(name + ".num_batches_tracked", params.get(name + ".num_batches_tracked", _ZERO_LONG)).detach().to(cx.dev)
                                   for name, _x in items], 1)
        for k, (name, x) in enumerate(items):
            rm, rv = rms[k], rvs[k]
            n = x.shape[0]
            if self.sync_bn:
                stats = merged[k]
                n = self._global_rows(x.shape[0], b)
                rm.mul_(1 - BN_MOMENTUM).add_(BN_MOMENTUM * stats[0])
                rv.mul_(1 - BN_MOMENTUM).add_(BN_MOMENTUM * stats[1] * (n / max(n - 1, 1)))
                self._bn_count[name] = n
            else:
                stats = ops.bn_stats(x, rm, rv, BN_MOMENTUM)
            new_stats[name + ".running_mean"], new_stats[name + ".running_var"] = rm, rv
            new_stats[name + ".num_batches_tracked"] = nbts[k]
            if self._bn_log is not None:
                self._bn_log.append((name, stats[0], stats[1], n))
            out.append(stats)
        return out

    def _replay_bn(self, log, new_stats):
        """The running-buffer updates of a forward whose WavEncoder pass is SHARED with an earlier forward of the step (same audio, same
        weights: same batch statistics): momentum update and batch counter of every BatchNorm once more, from the logged statistics."""
        params = self._params()
        dev = self.model.device
        names = [e[0] for e in log]
        rms = [new_stats.get(n + ".running_mean", params[n + ".running_mean"]).detach().to(dev, torch.float32) for n in names]
        rvs = [new_stats.get(n + ".running_var", params[n + ".running_var"]).detach().to(dev, torch.float32) for n in names]
        rms = torch._foreach_mul(rms, 1 - BN_MOMENTUM)
        torch._foreach_add_(rms, [e[1] for e in log], alpha=BN_MOMENTUM)
        rvs = torch._foreach_mul(rvs, 1 - BN_MOMENTUM)
        torch._foreach_add_(rvs, torch._foreach_mul([e[2] for e in log], [BN_MOMENTUM * e[3] / max(e[3] - 1, 1) for e in log]))
        nbts = torch._foreach_add([new_stats.get(n + ".num_batches_tracked", params.get(n + ".num_batches_tracked", _ZERO_LONG)).detach().to(dev) for n in names], 1)
        for n, rm, rv, nbt in zip(names, rms, rvs, nbts):
            new_stats[n + ".running_mean"], new_stats[n + ".running_var"], new_stats[n + ".num_batches_tracked"] = rm, rv, nbt

    def _wav_encoders(self, cx, encs, audio, b, new_stats):
        """WavEncoder.forward (P:296-314) with train-mode BatchNorm for several encoders IN LOCK STEP (encs = [(name, index)]): block by
        block, so that the BatchNorm statistics of a stage — every encoder's bn1, then every encoder's bn2 and shortcut BatchNorm — form one
        exchange under sync_bn.  -> ([features (B*T', audio_f) fp32 per encoder], T')."""
        m = self.model
        blocks = m._wav_blocks()
        lens = m._wav_lengths(audio.shape[1])
        k, q = _WAV_TAPS, blocks[0][1]
        w_in = cx.pk.w["train.wav_in"]
        xs, lin = [None] * len(encs), None
        for i, (cin, cout, stride, pad, ds) in enumerate(blocks):
            bases = [f"{enc}.feat_extractor.{i}" for enc, _e in encs]
            lout = lens[i]
            rows = b * lout
            ys = []
            for (enc, e), base, x in zip(encs, bases, xs):
                if i == 0:
                    r = slice(e * 2 * q, (e + 1) * 2 * q)
                    y = torch.empty(rows, 2 * q, dtype=torch.float32, device=cx.dev)
                    ops.wav_conv_in(F32, audio, w_in["w"][r], w_in["b"][r], cx.pk.w["train.ones"][:2 * q], y, lout, stride, pad)
                else:
                    ent = cx.pk.w[base + ".conv1.raw"]
                    y, _ = cx.gemm(x, base + ".conv1.raw", conv=(stride, pad, lin, lout), m=rows, n_store=_rup(ent["n"]))
                ys.append(y)
            c1s = [y[:, :cout] for y in ys]
            st1s = self._bn_many(cx, [(base + ".bn1", c1) for base, c1 in zip(bases, c1s)], b, new_stats)
            c2s, y1s = [], []
            for base, c1, st1 in zip(bases, c1s, st1s):
                g1, b1 = cx.pk.w[base + ".bn1.affine"]
                y1 = torch.empty(rows, _rup(cout), dtype=torch.float32, device=cx.dev)
                if y1.shape[1] != cout:
                    y1.zero_()                             # padded channels feed conv2's contraction: they must be zero
                ops.bn_apply(c1, st1, g1, b1, y1[:, :cout], slope=0.01)
                c2, _ = cx.gemm(y1, base + ".conv2.raw", conv=(1, k // 2, lout, lout), m=rows, n_store=_rup(cout))
                c2s.append(c2[:, :cout])
                y1s.append(y1)
            items = []
            for base, c2, y in zip(bases, c2s, ys):        # P:287-290: bn2, then the shortcut's BatchNorm — independent of each other
                items.append((base + ".bn2", c2))
                if ds:
                    items.append((base + ".downsample.1", y[:, cout:2 * cout]))
            sts = self._bn_many(cx, items, b, new_stats)
            saved_all, outs = [], []
            for j, (base, c2, y, y1, c1, st1, x) in enumerate(zip(bases, c2s, ys, y1s, c1s, st1s, xs)):
                g2, b2 = cx.pk.w[base + ".bn2.affine"]
                out = torch.empty(rows, cout, dtype=torch.float32, device=cx.dev)
                cds, std = None, None
                if ds:
                    st2, std = sts[2 * j], sts[2 * j + 1]
                    cds = y[:, cout:2 * cout]
                    gd, bd = cx.pk.w[base + ".downsample.1.affine"]
                    ops.bn_apply(c2, st2, g2, b2, out, slope=0.01, sc=cds, sc_bn=(*std, gd, bd))
                else:
                    st2 = sts[j]
                    ops.bn_apply(c2, st2, g2, b2, out, slope=0.01, sc=x[:, :cout])
                outs.append(out)
                saved_all.append(dict(i=i, base=base, geom=(cin, cout, stride, pad, ds), x_prev=x, lin=lin, lout=lout, b=b, audio=audio, c1=c1, st1=st1,
                                      y1=y1[:, :cout], c2=c2, st2=st2, cds=cds, std=std, out=out))
            if self.tape is not None:
                self.tape.node(lambda svs=saved_all: self._wav_blocks_backward(cx, svs))
            xs, lin = outs, lout
        return xs, lens[-1]

    def _wav_encoder(self, cx, enc, e, audio, b, new_stats):
        """One encoder alone (tests; the step runs both in lock step through `_wav_encoders`)."""
        xs, ta = self._wav_encoders(cx, [(enc, e)], audio, b, new_stats)
        return xs[0], ta

    def _bn_backward_many(self, items):
        """Training-mode BatchNorm backward of several INDEPENDENT BatchNorms: items = [(name, x, stats, dy)] -> [dx]; parameter gradients
        are accumulated.  sync_bn: the per-channel sums of ALL items are summed over the ranks in ONE all-reduce (local sums -> parameter
        gradients, averaged later with all the others; their sum over ranks -> the input gradients)."""
        out = []
        if self.sync_bn:
            from . import dist as pdist
            sums = [ops.bn_backward_sums(x, stats, dy) for _name, x, stats, dy in items]
            tot = pdist.sum_over_group([t.clone() for pair in sums for t in pair], group=self.group)
        for k, (name, x, stats, dy) in enumerate(items):
            gamma = self._param(name + ".weight").float()
            if self.sync_bn:
                dg, db = sums[k]
                dx = ops.bn_backward_apply(x, stats, gamma, dy, (tot[2 * k], tot[2 * k + 1]), self._bn_count[name])
            else:
                dx, dg, db = ops.bn_backward(x, stats, gamma, dy)
            self._param_grad(name + ".weight", slice(None), dg)
            self._param_grad(name + ".bias", slice(None), db)
            out.append(dx)
        return out

    def _wav_blocks_backward(self, cx, svs):
        """BasicBlock.forward (P:283-294) backwards for the same block of several encoders in lock step: LeakyReLU, [bn2 and the
        (batch-normalised) shortcut of every encoder: one exchange], conv2, LeakyReLU, [bn1 of every encoder: one exchange], conv1
        (+ shortcut conv)."""
        tape = self.tape
        svs = [sv for sv in svs if tape.get(sv["out"]) is not None]
        if not svs:
            return
        k = _WAV_TAPS
        dvs = [ops.act_backward(tape.get(sv["out"]), sv["out"], 0.01) for sv in svs]
        items = []
        for sv, dv in zip(svs, dvs):
            items.append((sv["base"] + ".bn2", sv["c2"], sv["st2"], dv))
            if sv["geom"][4]:
                items.append((sv["base"] + ".downsample.1", sv["cds"], sv["std"], dv))
        dxs = iter(self._bn_backward_many(items))
        dc2s, dcdss = [], []
        for sv, dv in zip(svs, dvs):
            cin, cout, stride, pad, ds = sv["geom"]
            dc2s.append(next(dxs))
            dcdss.append(next(dxs) if ds else None)
            if not ds:
                tape.add(sv["x_prev"], dv, cols=cout)
        pre1 = []
        for sv, dc2 in zip(svs, dc2s):
            cin, cout, stride, pad, ds = sv["geom"]
            base, b, lout = sv["base"], sv["b"], sv["lout"]
            dy1 = self._conv_backward(cx, sv["y1"], cout, [(base + ".conv2.weight", base + ".conv2.bias")], dc2, k, 1, k // 2, lout, lout, b, True)
            pre1.append(ops.act_backward(dy1, sv["y1"], 0.01))
        dc1s = self._bn_backward_many([(sv["base"] + ".bn1", sv["c1"], sv["st1"], g) for sv, g in zip(svs, pre1)])
        for sv, dc1, dcds in zip(svs, dc1s, dcdss):
            self._wav_block_conv1_backward(cx, sv, dc1, dcds)

    def _wav_block_conv1_backward(self, cx, sv, dc1, dcds):
        tape = self.tape
        cin, cout, stride, pad, ds = sv["geom"]
        base, k, b, lin, lout = sv["base"], _WAV_TAPS, sv["b"], sv["lin"], sv["lout"]
        origins = [(base + ".conv1.weight", base + ".conv1.bias")]
        dys = dc1
        if ds:
            origins.append((base + ".downsample.0.weight", base + ".downsample.0.bias"))
            dys = torch.cat([dc1, dcds], 1)
        if sv["i"] == 0:
            if self.h2_backward:       # the first layer's weight gradient (Cin = 1) as ONE split-fp16 contraction over all positions (split-K)
                audio = sv["audio"]
                m = dys.shape[0]
                mp = _rup(m)
                dys_t = ops.h2_cast(dys, mp, scale=self.grad_scale, transpose=True)                         # (2*cout, mp)
                col = ops.im2col_t_h2(audio.reshape(-1, 1), 1, k, stride, pad, audio.shape[1], lout, b, mp)  # (k, mp)
                dw = torch.empty(dys.shape[1], _rup(k, 4), dtype=torch.float32, device=cx.dev)[:, :k]
                ops.gemm(H2, dys_t, col, None, None, None, None, dw, None, n=k, cp=mp, w_scale=16.0, a_scale=16.0 * self.grad_scale, workspace=self._splitk_ws(cx.dev))
            else:
                dw = ops.wav_conv_in_backward(dys, sv["audio"], lout, k, stride, pad)      # (2*cout, k): conv1 rows, then the shortcut conv's
            db = ops.col_sum(dys)
            for j, (wn, bn) in enumerate(origins):
                self._param_grad(wn, slice(None), dw[j * cout:(j + 1) * cout].view(cout, 1, k))
                self._param_grad(bn, slice(None), db[j * cout:(j + 1) * cout])
        else:
            tape.add(sv["x_prev"], self._conv_backward(cx, sv["x_prev"], cin, origins, dys, k, stride, pad, lin, lout, b, True), cols=cin)

    def _motion_encoder(self, cx, x0, t, b, cin0):
        return self._conv_encoder(cx, "motion_encoder", x0, t, b, cin0, spec.MOTION_ENC_LAYERS)

    # ---- differentiable pieces: each wrapper launches the forward op and, when a tape is attached, records its backward -----------
    def _drop_add(self, cx, o, masks, t, res=None):
        """res + dropout(o) with the mask the reference draws on the (T, B, C) tensor."""
        m, c = o.shape
        mk = masks.take((t, m // t, c), lazy=True).view(m, c)
        return self._mul_add(o, mk, res, t_rows=t)

    def _mha(self, cx, masks, q_src, k_src, v_src, k_rows, vt, vt_rows, b, tq, tk):
        """Attention with probability dropout.  *_src = (tensor-or-token the operand is a column block of, first column); q / k
        operand views are built here.  k_rows: the row buffer holding the keys."""
        d, h = self.model.config.hidden_size, spec.N_HEAD
        q = q_src[2]
        k = k_rows
        pm = masks.take((b, h, tq, tk))
        att = cx.lo(b * tq, d)
        ops.attention_dropout(cx.gdt, q, k, vt, vt_rows, att, b, h, tq, tk, d // h, pm)
        if self.tape is not None:
            def bw():
                g = self.tape.get(att)
                if g is None:
                    return
                # tokens (projections whose column blocks are all attention operands) are covered block by block by the attention
                # backwards of their layers: no zero fill; a real tensor (the cross-attention query) may have other consumers
                gq = self.tape.buffer(q_src[0], zero=not isinstance(q_src[0], _Token))[:, q_src[1]:q_src[1] + d]
                gk = self.tape.buffer(k_src[0], zero=not isinstance(k_src[0], _Token))[:, k_src[1]:k_src[1] + d]
                gv = self.tape.buffer(v_src[0], zero=not isinstance(v_src[0], _Token))[:, v_src[1]:v_src[1] + d]
                ops.attention_backward(q, k, vt, vt_rows, pm, g, gq, gk, gv, b, h, tq, tk, d // h)
            self.tape.node(bw)
        return att

    def _self_attn(self, cx, masks, name, x, b, t):
        d = self.model.config.hidden_size
        qk, vt, tok = self._lin_kv(cx, x, name + ".sa.qkv", 2 * d, t, b)
        att = self._mha(cx, masks, (tok, 0, qk[:, :d]), (tok, d), (tok, 2 * d), qk[:, d:], vt, d, b, t, t)
        o = self._lin(cx, att, name + ".sa.out")
        return self._drop_add(cx, o, masks, t, res=x)

    def _ffn(self, cx, masks, name, x, t):
        f = self._lin(cx, x, name + ".ff1", slope=0.0)
        f = self._drop_add(cx, f, masks, t)
        o = self._lin(cx, f, name + ".ff2")
        return self._drop_add(cx, o, masks, t, res=x)

    def _encoder_layer(self, cx, masks, name, x, b, t):
        x = self._layernorm(cx, name + ".norm1", self._self_attn(cx, masks, name, x, b, t))
        return self._layernorm(cx, name + ".norm2", self._ffn(cx, masks, name, x, t))

    def _decoder_layer(self, cx, masks, name, x, b, t, mem, vt_rows, tk):
        """mem = (keys as rows, V^T buffer view, token of the K/V projection, first K column, first V column)."""
        d = self.model.config.hidden_size
        mem_k, mem_vt, tok, kc, vc = mem
        x = self._layernorm(cx, name + ".norm1", self._self_attn(cx, masks, name, x, b, t))
        q = self._lin(cx, x, name + ".ca.q")
        att = self._mha(cx, masks, (q, 0, q), (tok, kc), (tok, vc), mem_k, mem_vt, vt_rows, b, t, tk)
        o = self._lin(cx, att, name + ".ca.out")
        x = self._layernorm(cx, name + ".norm2", self._drop_add(cx, o, masks, t, res=x))
        return self._layernorm(cx, name + ".norm3", self._ffn(cx, masks, name, x, t))

    def _memory(self, cx, key, mem_rows, b, tk, n_layers):
        """K / V projection of a cross-attention memory for n_layers layers: per layer the tuple `_decoder_layer` takes."""
        d = self.model.config.hidden_size
        k, vt, tok = self._lin_kv(cx, mem_rows, key, n_layers * d, tk, b)
        return [(k[:, i * d:(i + 1) * d], vt[:, i * d:], tok, i * d, n_layers * d + i * d) for i in range(n_layers)]

    def _ppe(self, cx, masks, x, b, t):
        """PeriodicPositionalEncoding.forward (P:341-343): dropout(x + pe[:, :T]) on (B*T, d) rows."""
        m, d = x.shape
        y = self._add(cx, x, cx.pk.w["pe"][:t], mod_b=t)
        return self._mul_add(y, masks.take((b, t, d), lazy=True).view(m, d))

    def _speaker(self, cx, key, name, sid):
        rows = ops.gather_rows(cx.pk.w[key], sid, F32)
        if self.tape is not None:
            def bw():
                g = self.tape.get(rows)
                if g is None:
                    return
                n_rows = cx.pk.w[key].shape[0]
                if n_rows == 1:                           # one speaker: every clip read row 0
                    self._param_grad(name, slice(None), ops.col_sum(g))
                else:                                     # per-clip ids: each table row takes the clips that read it (clamped as the gather clamps)
                    self._param_grad(name, slice(None), ops.embedding_backward(g, sid[:, 0], n_rows))
            self.tape.node(bw)
        return rows

    # ---- the forward --------------------------------------------------------------------------------------------------------
    def __call__(self, audio, speaker_id, masked_motion, mask, dropout_masks=None, use_audio=True, new_stats=None, tape=False, rng=None, share=None):
        """-> (dict of the 8 (B, T, 256) fp32 outputs, new_stats).  `new_stats` carries the BatchNorm running buffers from one
        forward of a step to the next (as oracle.emage_train_oracle.forward_train does); it is not written into the model.
        tape=True keeps what `backward()` needs (see there).  dropout_masks None: the masks are drawn on the device from
        rng = (seed, step, first mask id) — see `_Masks`.  share: the `StepShare` of the optimisation step this forward belongs to
        (same audio and weights as the step's other forwards): the WavEncoder pass is computed by the first of them only."""
        model = self.model
        c = model.config
        # the training forward keeps float32 activations (split inside the GEMMs in f16x3); train_only: the operand set leaves out what
        # only the eval-mode forward reads (the WavEncoder convolutions with their BatchNorms folded in)
        cx = _Ctx(model._engine(h2=False, train_only=True))
        pk, dev = cx.pk, cx.dev
        self._train_pack(pk)
        self._begin_forward(cx, tape)            # (inside a `Trainer` step the weights are those of the step's first forward: the images stay)
        new_stats = {} if new_stats is None else new_stats
        if self.sync_bn and share is None and not _capturing(dev):      # a forward outside a `Trainer` step (the class API): the global clip
            self._clips.clear()                                         # count is exchanged afresh (see `_clip_total`; a step: `begin_step`)
        masks = _Masks(dropout_masks, dev, rng, lazy=self.lazy_masks, needs=dropout_mask_count())
        b, t, cm = masked_motion.shape
        m = b * t
        d, mf, af = c.hidden_size, c.motion_f, c.audio_f
        nf, nc = spec.N_FACE_LAYERS, spec.N_CROSS_LAYERS
        audio = audio.to(device=dev, dtype=torch.float32).contiguous()
        motion3 = masked_motion.to(device=dev, dtype=torch.float32).contiguous()
        mask3 = mask.to(device=dev, dtype=torch.float32).contiguous()

        # masked motion -> spatial hints (M:267-273)
        x0 = ops.pack_motion(cx.dt, motion3, mask3, pk.w["mask_emb"], _rup(cm))
        if self.tape is not None:
            def bw_mask_embedding():                                                 # x0 = mask ? mask_embedding : motion (M:267-268)
                g = self.tape.get(x0)
                if g is not None:
                    self._param_grad("mask_embedding", slice(None), ops.col_sum(g[:, :cm], mask3.view(m, cm)))
            self.tape.node(bw_mask_embedding)
        hint = self._motion_encoder(cx, x0, t, b, cm)
        hh = self._lin(cx, hint, "bodyhints.fc1", slope=0.1)
        memcat = cx.lo(m, af + mf)                                                   # [audio2face | body_hint_face] (M:288)
        hh_face, hh_body = hh[:, :d], hh[:, d:]
        hint_face = memcat[:, af:]
        if self.tape is not None:
            self.tape.view(hh, hh_face, 0)
            self.tape.view(hh, hh_body, d)
            self.tape.view(memcat, hint_face, af, written=True)
        self._lin(cx, hh_face, "bodyhints_face.fc2", out=hint_face)
        hint_body = self._lin(cx, hh_body, "bodyhints_body.fc2")

        # the two WavEncoders, batch statistics (M:275-281), block by block in lock step; shared by the forwards of a step
        self._shared = share
        if share is not None and share.feats is not None:
            a_face, a_body, ta = share.feats
            self._replay_bn(share.bn_log, new_stats)
        else:
            main = self.tape
            if share is not None:
                self._bn_log = share.bn_log
                if main is not None:
                    self.tape = share.tape = _Tape(dev)      # the encoders' backward waits for the gradients of all the step's forwards
            try:
                (a_face, a_body), ta = self._wav_encoders(cx, [("audio_encoder_face", 0), ("audio_encoder_body", 1)], audio, b, new_stats)
            finally:
                self.tape, self._bn_log = main, None
            if share is not None:
                share.feats = (a_face, a_body, ta)
        if ta < t:
            raise RuntimeError(f"Sizes of tensors must match: audio features {ta} frames vs motion {t} frames")
        memcat[:, :af] = a_face.view(b, ta, af)[:, :t].reshape(m, af)                # M:278-281: the FACE features are trimmed to T
        if self.tape is not None:
            def bw_face_features():
                g = self.tape.get(memcat)
                if g is None:
                    return
                ga = torch.zeros(b, ta, af, dtype=torch.float32, device=dev)
                ga[:, :t] = g[:, :af].reshape(b, t, af)
                self.tape.add(a_face, ga.view(b * ta, af))
            self.tape.node(bw_face_features)

        sid = speaker_id.to(dev).reshape(b, 1).expand(b, t)
        spk_body = self._speaker(cx, "spk_body", "speaker_embedding_body.weight", sid)
        spk_face = self._speaker(cx, "spk_face", "speaker_embedding_face.weight", sid)
        out = {}

        # face branch (M:288-294)
        mem_face = self._lin(cx, memcat, "audio_face_motion_proj")
        face = self._ppe(cx, masks, spk_face, b, t)
        fmem = self._memory(cx, "face.kv_all", mem_face, b, t, nf)
        for i in range(nf):
            face = self._decoder_layer(cx, masks, f"face_motion_decoder.layers.{i}", face, b, t, fmem[i], nf * d, t)
        out["rec_face"] = self._lin(cx, face, "face_out_proj")
        out["cls_face"] = self._lin(cx, self._lin(cx, out["rec_face"], "face_cls.fc1", slope=0.1), "face_cls.fc2")

        # body branch (M:297-312)
        x = self._ppe(cx, masks, self._lin(cx, hint_body, "moton_proj"), b, t)
        x = self._encoder_layer(cx, masks, "motion_self_encoder.layers.0", self._add(cx, x, spk_body), b, t)
        mem_body = self._lin(cx, a_body, "audio_body_motion_proj")                   # M:303
        base = self._ppe(cx, masks, self._add(cx, x, spk_body), b, t)               # M:304-305
        x = base
        bmem = self._memory(cx, "cross.kv_all", mem_body, b, ta, nc)
        for i in range(nc):
            x = self._decoder_layer(cx, masks, f"audio_motion_cross_attn.layers.{i}", x, b, t, bmem[i], nc * d, ta)
        fea = self._add(cx, base, x) if use_audio else base                          # motion_fea + cross; cross * 0 without audio (M:310-312)

        # part latents, refinement layers, heads (M:315-330)
        parts = ("upper", "hands", "lower")
        others = {"upper": ("hands", "lower"), "hands": ("upper", "lower"), "lower": ("upper", "hands")}
        hl = self._lin(cx, fea, "motion2latent.fc1", slope=0.1)
        lat = {}
        for i, p in enumerate(parts):
            hv = hl[:, i * d:(i + 1) * d]
            if self.tape is not None:
                self.tape.view(hl, hv, i * d)
            lat[p] = self._lin(cx, hv, f"motion2latent_{p}.fc2")
        refine = {}
        for p in parts:
            tgt = self._add(cx, lat[p], spk_body)
            mem_lo = self._add(cx, lat[others[p][0]], lat[others[p][1]])
            name = f"body_motion_decoder_{p}.layers.0"
            refine[p] = self._decoder_layer(cx, masks, name, tgt, b, t, self._memory(cx, name + ".ca.kv", mem_lo, b, t, 1)[0], d, t)
        for p in parts:
            out[f"rec_{p}"] = self._lin(cx, self._add(cx, lat[p], refine[p]), f"motion_out_proj_{p}")
        for p in parts:
            out[f"cls_{p}"] = self._lin(cx, self._lin(cx, out[f"rec_{p}"], f"motion_cls_{p}.fc1", slope=0.1), f"motion_cls_{p}.fc2")
        if not masks.consumed_all():
            raise RuntimeError(f"dropout_masks: {len(masks.masks)} masks given, the forward consumed {masks.i}")
        self._out2d = out
        return {key: out[key].view(b, t, -1) for key in OUT_KEYS}, new_stats

    # ---- backward through everything behind the motion encoder and the WavEncoders ------------------------------------------------
    def backward(self, index_gt, latent_gt, progress=None):
        """Gradients of `rec_loss + cls_loss` (T:106-130) of the LAST forward (called with tape=True) w.r.t. every trainable parameter
        that takes part in it; they ACCUMULATE in `self.param_grads` (name -> fp32 tensor of the parameter's shape) across the
        forwards of a step, like `loss_all.backward()` in the reference (T:174).  Every contraction (Linear and Conv1d, dX and dW) is
        an emage_gemm launch in exact-fp32 mode on transposed / im2col operands."""
        if self.tape is None:
            raise RuntimeError("backward() needs the forward to be run with tape=True")
        cfg, tape, out = self.model.config, self.tape, self._out2d
        for q in ("upper", "lower", "hands", "face"):
            pred = out[f"rec_{q}"]
            tape.add(pred, ops.mse_loss_grad(pred, latent_gt[q].reshape(pred.shape).to(pred.device), getattr(cfg, "l" + q[0])))
            logits = out[f"cls_{q}"]
            # cf = 0 in the reference's config: the face classifier's loss is evaluated and multiplied by 0 (T:113-128), its
            # parameters receive exact-zero gradients and an Adam state — kept that way
            tape.add(logits, ops.nll_loss_grad(logits, index_gt[q].reshape(-1).contiguous().to(logits.device), getattr(cfg, "c" + q[0])))
        tape.run(progress)
        self.flush_param_grads()
        self.last_run_nodes = tape.pos + 1
        share = self._shared
        if share is not None and share.tape is not None:           # the feature gradients of this forward join the shared encoder pass
            for feat in share.feats[:2]:
                g = tape.get(feat)
                if g is not None:
                    share.tape.add(feat, g)
        self.tape = None
        return self.param_grads

    def finish_shared(self, share, progress=None, base=0):
        """Backward of the step-shared WavEncoder pass from the summed feature gradients (call behind the step's last `backward`)."""
        if share is None or share.tape is None:
            return
        self.tape = share.tape
        try:
            share.tape.run(progress, base=base)
            self.flush_param_grads()
        finally:
            self.tape = None
        share.tape = None

    def backward_from(self, tape, out2d, grad_outputs):
        """Backward of ONE recorded forward from the gradients of its outputs (the autograd bridge of the model classes' train-mode
        forward: torch computes d loss / d output, this runs the rest): returns {parameter name: gradient} of that forward alone."""
        self.tape = tape
        try:
            with self.grads.alone() as own:              # (an exception mid-walk: what was queued is dropped)
                for key, g in grad_outputs.items():
                    if g is not None:
                        t = out2d[key]
                        tape.add(t, g.reshape(t.shape).to(torch.float32).contiguous())
                tape.run()
            return own
        finally:
            self.tape = None


# ======================================================================================
# the autograd bridge: `model.train(); out = model(audio, speaker_id, masked_motion, mask); loss.backward()` (T:156-181)
# ======================================================================================
class _TrainFn(torch.autograd.Function):
    """One train-mode forward of an EmageAudioModel as ONE autograd node: forward = `TrainForward.__call__` with a tape, backward =
    the tape run from the gradients torch hands in for the eight outputs.  The trainable parameters are inputs of the node, so
    `.grad` accumulation, optimisers and hooks behave as for the reference module."""

    @staticmethod
    def forward(ctx, fwd, names, audio, speaker_id, masked_motion, mask, use_audio, dropout_masks, rng, *params):
        with torch.no_grad():
            pred, stats = fwd(audio, speaker_id, masked_motion, mask, dropout_masks, use_audio=use_audio, tape=True, rng=rng)
            flat = fwd.model._flat_params()
            for name, v in stats.items():                 # train-mode BatchNorm: the running buffers advance in place, as in torch
                if name in flat:
                    flat[name].copy_(v.to(flat[name].dtype))
        ctx.fwd, ctx.names, ctx.tape, ctx.out2d = fwd, names, fwd.tape, fwd._out2d
        fwd.tape = None
        return tuple(pred[k] for k in OUT_KEYS)

    @staticmethod
    def backward(ctx, *grad_outputs):
        grads = ctx.fwd.backward_from(ctx.tape, ctx.out2d, dict(zip(OUT_KEYS, grad_outputs)))
        ctx.tape = None
        return (None,) * 9 + tuple(grads.get(n) for n in ctx.names)


def train_forward(model, audio, speaker_id, masked_motion, mask, use_audio=True):
    """EmageAudioModel.forward in TRAINING mode (what `model(...)` runs after `model.train()`): differentiable w.r.t. the model's
    parameters through `_TrainFn`.  Dropout masks come from the device generator (seeded by `torch.initial_seed()`, advancing with
    every call) unless `model.dropout_masks_override` holds recorded mask lists (the parity tests), consumed one per call."""
    fwd = model.__dict__.get("_train_fwd")
    if fwd is None:
        fwd = model.__dict__["_train_fwd"] = TrainForward(model)
        model.__dict__["_train_calls"] = 0
    # an optimiser step (or any in-place edit of a parameter / BatchNorm buffer) since the last forward is seen by `model._engine()`
    # itself (`_version_stamp`), in train and in eval mode: the packed operands are rebuilt from the current parameters
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    override = getattr(model, "dropout_masks_override", None)
    masks = override.pop(0) if override else None
    model.__dict__["_train_calls"] += 1
    rng = (int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF, model.__dict__["_train_calls"], 0)
    outs = _TrainFn.apply(fwd, [n for n, _p in named], audio, speaker_id, masked_motion, mask, bool(use_audio), masks, rng, *[p for _n, p in named])
    return dict(zip(OUT_KEYS, outs))


# ======================================================================================
# the three forwards of a step and their six losses (train_emage_audio.py:132-172)
# ======================================================================================
def targets(vq, motion_aa, expressions, trans, foot_contact):
    """Top of train_val_fn (T:146-152): axis-angle -> rot-6D, the frozen VQ-VAEs' code indices and quantised latents, and the
    337-channel motion the model is conditioned on — all on the device (`vq` is the product EmageVQModel)."""
    bs, t, jc = motion_aa.shape
    dev = vq.vq_model_face.device
    aa = motion_aa.to(device=dev, dtype=torch.float32).reshape(bs * t * (jc // 3), 3).contiguous()
    rot6d = ops.axis_angle_to_rot6d(aa).reshape(bs, t, jc // 3 * 6)
    expressions, trans, foot_contact = (x.to(device=dev, dtype=torch.float32) for x in (expressions, trans, foot_contact))
    index = vq.map2index(rot6d, expressions, tar_contact=foot_contact, tar_trans=trans)
    latent = vq.map2latent(rot6d, expressions, tar_contact=foot_contact, tar_trans=trans)
    return index, latent, torch.cat([rot6d, trans, foot_contact], dim=-1)


def losses(cfg, pred, index_gt, latent_gt, workspace=None):
    """(rec, cls) of T:106-130 as float64 device scalars: sum_q l_q * mse(rec_q, latent_q), sum_q c_q * NLL(log_softmax(cls_q), index_q)."""
    dev = pred["rec_face"].device
    ws = ops.loss_workspace(dev) if workspace is None else workspace
    rec, cls = torch.zeros(1, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
    for q in ("upper", "lower", "hands", "face"):
        b, t, k = pred[f"rec_{q}"].shape
        ops.mse_loss(pred[f"rec_{q}"].reshape(b * t, k), latent_gt[q].reshape(b * t, k), getattr(cfg, "l" + q[0]), rec, ws)
        ops.nll_loss(pred[f"cls_{q}"].reshape(b * t, -1), index_gt[q].reshape(-1).contiguous(), getattr(cfg, "c" + q[0]), cls, ws)
    return rec, cls


def speaker_ids(speaker_id, bs, device, speaker_dims=None):
    """The (B, 1) int64 device tensor of per-clip speaker-table rows a step's forwards read.  None: zeros (the reference's scripts,
    T:146).  A (B, 1) / (B,) int64 tensor already on the device is used IN PLACE (a captured step reads the caller's buffer at every
    replay).  speaker_dims: a host-visible tensor is checked against it (ValueError for a row outside [0, speaker_dims)); device tensors
    are not read back — the store that produced them validated its rows (`data.ClipLoader(speaker_dims=...)`), and the kernels clamp."""
    device = torch.device(device)
    if speaker_id is None:
        return torch.zeros(bs, 1, dtype=torch.long, device=device)
    if not torch.is_tensor(speaker_id):
        speaker_id = torch.as_tensor(speaker_id)
    if speaker_id.dtype != torch.int64 or speaker_id.numel() != bs or speaker_id.dim() not in (1, 2) or (speaker_id.dim() == 2 and speaker_id.shape[1] != 1):
        raise ValueError(f"speaker_id must be a (B, 1) or (B,) int64 tensor with B = {bs}, not {tuple(speaker_id.shape)} {speaker_id.dtype}")
    if speaker_dims is not None and not speaker_id.is_cuda and bs:
        lo, hi = int(speaker_id.min()), int(speaker_id.max())
        if lo < 0 or hi >= speaker_dims:
            raise ValueError(f"speaker_id holds rows in [{lo}, {hi}]; the model's speaker tables have {speaker_dims} rows (speaker_dims)")
    return speaker_id.to(device).reshape(bs, 1)


def step_losses(fwd: TrainForward, vq, batch, iteration, dropout_masks, random_mask, speaker_id=None):
    """The seed / audio / mask forwards of one step (T:132-172) -> (dict of the six losses + "all" as Python floats, BatchNorm
    buffers after the three forwards).  dropout_masks: three mask lists (one per forward); random_mask: the (B, T, 337)
    {0, 1} motion mask of forwards 2 and 3, `torch.rand(...) < mask_ratio` in the reference (T:163-165).  speaker_id: per-clip rows of
    the speaker tables (`speaker_ids`); None = zeros."""
    cfg = fwd.model.config
    index, latent, masked_motion = targets(vq, batch["motion"], batch["expressions"], batch["trans"], batch["foot_contact"])
    bs, t = masked_motion.shape[:2]
    speaker_id = speaker_ids(speaker_id, bs, masked_motion.device, cfg.speaker_dims)
    seed_mask = torch.ones_like(masked_motion)
    seed_mask[:, :cfg.seed_frames] = 0
    stats, out = {}, {}
    ws = ops.loss_workspace(masked_motion.device)
    for tag, mask, use_audio, masks in (("seed", seed_mask, True, dropout_masks[0]), ("audio", random_mask, True, dropout_masks[1]),
                                        ("mask", random_mask, False, dropout_masks[2])):
        pred, stats = fwd(batch["audio"], speaker_id, masked_motion, mask, masks, use_audio=use_audio, new_stats=stats)
        out["rec_" + tag], out["cls_" + tag] = losses(cfg, pred, index, latent, ws)
    res = {k: float(v) for k, v in out.items()}
    ops.loss_check(ws)
    res["all"] = sum(res.values())
    return res, stats


_CLIP_TABLES = {}                                         # ((gradient pointer, n), ...) -> ops.AdamTable: valid exactly as long as the key matches


def _clip_table(grads):
    """The pointer table over `grads` for `clip_grad_norm_`, cached per set of (pointer, n): a table stays right for as long as the
    gradients sit where they sat (an optimizer.zero_grad() that frees them usually hands the same blocks back).  It holds no reference to
    the gradients; a handful of sets are kept."""
    key = tuple((g.data_ptr(), g.numel()) for g in grads)
    tab = _CLIP_TABLES.get(key)
    if tab is None:
        while len(_CLIP_TABLES) >= 8:
            _CLIP_TABLES.pop(next(iter(_CLIP_TABLES)))
        tab = _CLIP_TABLES[key] = ops.AdamTable([(g, g, g, g) for g in grads], grads[0].device)      # only the gradient word and n are read
        tab.keep = None
    return tab


def clip_grad_norm_(parameters, max_norm):
    """torch.nn.utils.clip_grad_norm_(parameters, max_norm) (norm_type 2) on the device for the reference-style loop — `loss.backward();
    clip_grad_norm_(model.parameters(), cfg.max_grad_norm); optimizer.step()`: one sum-of-squares launch (float64, fixed order) and one
    scaling launch over the `.grad` of the given parameters (contiguous fp32 on the device; parameters without a gradient are skipped).
    Returns the total norm as a 0-dim fp32 DEVICE tensor — no host synchronisation."""
    params = [parameters] if torch.is_tensor(parameters) else list(parameters)
    grads = [p.grad for p in params if p.grad is not None and p.grad.numel()]
    if not grads:
        return torch.zeros((), dtype=torch.float32, device=params[0].device if params else None)
    for g in grads:
        if not (g.is_cuda and g.dtype == torch.float32 and g.is_contiguous()):
            raise RuntimeError("clip_grad_norm_: gradients must be contiguous fp32 tensors on the device (no CPU fallback)")
    tab = _clip_table(grads)
    out = ops.grad_norm(tab, 1.0, max_norm)
    ops.scale_multi(tab, out.coef)
    return out.norm.clone().reshape(())


class Trainer:
    """One optimisation step of train_emage_audio.py:132-180 on the device: the three train-mode forwards with their backward
    passes (gradients accumulate like `loss_all.backward()`), torch.optim.Adam with the reference's settings (lr 1.5e-4 constant,
    betas .9 / .999, eps 1e-8, no weight decay: configs/emage_audio.yaml:63-78), the BatchNorm running buffers.  Parameters that
    take no part in the forward (the deep-copied template layers, M:246-262) get no gradient and stay untouched, as in torch.

    Gradients live in four flat, backward-ordered buckets (`dist.GradientBuckets`: the backward kernels' results are accumulated
    straight into the all-reduce messages, no copies).  In a multi-process run (`group` / an initialised default group) bucket i is
    all-reduced AS SOON AS its last gradient of the step has been written — during the third backward, while the remaining backward
    kernels are still being issued (the overlap DDP gives the reference, T:251): the tape position of every parameter's last
    contribution is learned during the first step (the launch sequence of a step is static) and drives the schedule from the second
    step on.  The 1 / world_size of the average is folded into Adam, which is ONE multi-tensor launch that also clears the gradients.
    Dropout masks: `dropout_masks` (three lists, the parity tests) or None = drawn on the device (`ops.dropout_mask`, seeded by `seed`).
    `grad_hook(param_grads)` still runs between backward and the update (tests spy on it)."""

    def __init__(self, model, vq, lr=1.5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, sync_bn=False, group=None, seed=0, exchange=True,
                 on_nonfinite="raise", share_encoders=True, exchange_dtype=torch.float32, max_grad_norm=None, track_grad_norm=False):
        """exchange=False: no built-in gradient all-reduce even in a multi-process run (a `grad_hook` may do it: `dist.gradient_allreduce_hook`).

        Health of a step (the f16x3 backward runs on fp16 planes of `grad_scale` x dY and of scaled weights: an overflow turns into
        inf / NaN): `emage_count_nonfinite` over the four gradient buckets runs INSIDE the step (eager and captured), in front of Adam, and
        Adam takes the count as its skip word — a poisoned step never reaches the parameters, the moments or the BatchNorm buffers.  The
        count travels to the host with the losses; on_nonfinite = "raise": FloatingPointError (the state is that of the previous step);
        "skip": the step is dropped (`skipped_steps`), `grad_scale` is halved and training goes on (a captured step is re-captured with
        the new scale: it is a launch argument) — the step-skip of loss-scaled mixed-precision training.  Weight operand scales are
        power-of-two constants chosen once; every re-packing checks on the device that max |w| x scale is still in [2^10, 2^14) and the
        trainer re-derives the scales behind the step that reports a miss (two doublings before an fp16 plane could overflow).

        max_grad_norm: clip the gradient by its global 2-norm (torch.nn.utils.clip_grad_norm_; configs/emage_audio.yaml:67) INSIDE the step,
        between the exchange and Adam — `ops.grad_norm` over the Adam table (float64 sums in a fixed order, pre_scale = 1 / world: the norm of
        the AVERAGED gradient, what DDP followed by clip_grad_norm_ sees) and the coefficient as Adam's device-side gradient factor; eager
        and captured.  track_grad_norm: the same launch without clipping.  Either adds "grad_norm" to the loss dict and fills
        `param_grad_norms()`; a skipped step reports its inf / NaN norm.  Both off (the default): no launch, the step is unchanged."""
        from . import dist as pdist
        if on_nonfinite not in ("raise", "skip"):
            raise ValueError("on_nonfinite must be 'raise' or 'skip'")
        self.on_nonfinite, self.skipped_steps, self.rescaled = on_nonfinite, 0, 0
        self.nonfinite_loss_steps = 0                     # steps whose loss was inf / NaN although every gradient was finite (update applied; see `_finish`)
        # share_encoders: the WavEncoder pass of a step is computed (and differentiated) once for its three forwards — see `StepShare`;
        # False = the reference's schedule, three passes (same losses; gradients equal up to fp32 summation order)
        self.share_encoders = bool(share_encoders)
        self.exchange = bool(exchange)
        self.fwd, self.vq = TrainForward(model, sync_bn=sync_bn, group=group), vq
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.group, self.seed = group, int(seed)
        self.state = {}                                   # name -> dict(step, exp_avg, exp_avg_sq)
        named = [(k, v) for k, v in model.named_parameters() if v.requires_grad]
        plan, self.unused = pdist.emage_bucket_plan(named)
        self.buckets = pdist.GradientBuckets(plan, device=model.device, group=group, exchange_dtype=exchange_dtype)       # bfloat16: half the bytes on the wire
        self.fwd.grad_views = self.buckets.grads
        self.bucket_of = {name: i for i, (_tag, params) in enumerate(plan) for name, _p in params}
        self.schedule = None                              # bucket -> tape position (third backward) behind which it is complete
        self.exchange_log = []                            # (event, bucket or tape position) of the last step: what the overlap tests read
        self.steps_done = 0
        self._adam = None
        self._graph, self._recapture_pending = None, False
        self.health = torch.zeros(1, dtype=torch.int32, device=model.device)       # non-finite gradient words of the last step (Adam's skip word)
        self._max_grad_norm = _check_max_norm(max_grad_norm)
        self.track_grad_norm = bool(track_grad_norm)
        self._grad_norm, self._adam_names = None, []      # `ops.GradNorm` of the last step (buffers of the Adam table), the table's parameter names

    @property
    def max_grad_norm(self):
        return self._max_grad_norm

    @max_grad_norm.setter
    def max_grad_norm(self, value):
        value = _check_max_norm(value)
        if value != self._max_grad_norm and self._graph is not None:      # a launch argument of the captured step, like the loss scale
            self._recapture_pending = True
        self._max_grad_norm = value

    def param_grad_norms(self):
        """{parameter name: 2-norm of its (averaged) gradient} of the last step — one device-to-host copy of the float64 sums of squares."""
        return _param_grad_norms(self._grad_norm, self._adam_names, 1.0 / self._world())

    def _world(self):
        import torch.distributed as tdist
        if not self.exchange:
            return 1
        return tdist.get_world_size(self.group) if (tdist.is_available() and tdist.is_initialized()) else 1

    def _exchanging(self):
        """True when the step runs its gradient exchange: a process group exists (and exchange=True) — ALSO at world size 1, like
        DistributedDataParallel: the four bucket all-reduces then go through the backend (RCCL on one MI355X: the only way to run the
        exchange on hardware without a multi-GPU node, tests/test_train_forward_gpu.py) and are the identity."""
        import torch.distributed as tdist
        return self.exchange and tdist.is_available() and tdist.is_initialized()

    def _rng(self, forward_index, step):
        return (self.seed, step, 128 * forward_index)

    def _device_step(self, batch, dropout_masks, random_mask, grad_hook=None, step_counter=None, speaker_id=None):
        """Everything of a step that runs on the device; returns (dict of float64 device loss scalars, loss workspace).  With
        `step_counter` (one int32 on the device) Adam and the mask generator read the step count from it — what a captured graph needs."""
        fwd, model = self.fwd, self.fwd.model
        cfg = model.config
        index, latent, masked_motion = targets(self.vq, batch["motion"], batch["expressions"], batch["trans"], batch["foot_contact"])
        bs = masked_motion.shape[0]
        speaker_id = speaker_ids(speaker_id, bs, masked_motion.device, cfg.speaker_dims)
        seed_mask = torch.ones_like(masked_motion)
        seed_mask[:, :cfg.seed_frames] = 0
        fwd.param_grads = {}
        try:
            with fwd.step():                              # a step that dies mid-backward: its queued contributions die with it
                return self._device_step_body(batch, dropout_masks, random_mask, grad_hook, step_counter, index, latent, masked_motion, speaker_id, seed_mask)
        except BaseException:
            for flat in self.buckets.flat:                # Adam's zero_grad never ran for the dead step
                flat.zero_()
            raise

    def _device_step_body(self, batch, dropout_masks, random_mask, grad_hook, step_counter, index, latent, masked_motion, speaker_id, seed_mask):
        fwd, model = self.fwd, self.fwd.model
        cfg = model.config
        stats, out = {}, {}
        ws = ops.loss_workspace(masked_motion.device)
        world, exchanging = self._world(), self._exchanging()
        buckets, log = self.buckets, []
        self.exchange_log = log
        learning = self.schedule is None
        step_for_rng = step_counter if step_counter is not None else self.steps_done + 1
        dm = dropout_masks if dropout_masks is not None else (None, None, None)
        share = StepShare() if self.share_encoders else None
        for f, (tag, mask, use_audio, masks) in enumerate((("seed", seed_mask, True, dm[0]), ("audio", random_mask, True, dm[1]),
                                                            ("mask", random_mask, False, dm[2]))):
            pred, stats = fwd(batch["audio"], speaker_id, masked_motion, mask, masks, use_audio=use_audio, new_stats=stats, tape=True,
                              rng=self._rng(f, step_for_rng), share=share)
            out["rec_" + tag], out["cls_" + tag] = losses(cfg, pred, index, latent, ws)
            progress = None
            if f == 2:
                if learning:
                    fwd.grads.touch = {}
                elif exchanging:
                    ready = {}
                    for i, pos in self.schedule.items():
                        ready.setdefault(pos, []).append(i)

                    def progress(pos, ready=ready):
                        for i in ready.get(pos, ()):         # every gradient of bucket i is final: its all-reduce overlaps the rest of the backward
                            fwd.flush_param_grads()          # ... once its queued contributions have been applied
                            log.append(("reduce", i, pos))
                            buckets.reduce(i)
            fwd.backward(index, latent, progress)
            if f == 2:                                    # the shared WavEncoder pass: the tail of the third backward
                fwd.finish_shared(share, progress, base=fwd.last_run_nodes)
            log.append(("backward_done", f))
        # non-finite LOSS words of this rank — in an exchanging run the MAXIMUM over ranks (one more small all-reduce; a graph node in a captured
        # step): a loss is rank-local, so without it `on_nonfinite="raise"` would raise on ONE rank and leave the others in their next collective
        self.loss_health = (~torch.isfinite(torch.stack([v.reshape(()) for v in out.values()]))).sum().to(torch.int32).reshape(1)
        if exchanging and world > 1:
            import torch.distributed as tdist
            tdist.all_reduce(self.loss_health, op=tdist.ReduceOp.MAX, group=self.group)
        if learning:
            last = {}
            for name, pos in fwd.grads.touch.items():
                i = self.bucket_of[name]
                last[i] = max(last.get(i, -1), pos)
            self.schedule = {i: last.get(i, -1) for i in range(len(buckets.flat))}      # -1: complete before the third backward starts
            fwd.grads.touch = None
            if exchanging:
                for i in range(len(buckets.flat)):
                    log.append(("reduce", i, None))
                    buckets.reduce(i)
        grads = fwd.param_grads
        if exchanging:
            buckets.wait(average=False)                   # the 1 / world of the average is Adam's grad_scale
            log.append(("wait",))
        if grad_hook is not None:
            grad_hook(grads)
        fwd.flush_range_checks(new_step=True)
        # health: inf / NaN among the (exchanged) gradients -> Adam's skip word.  After the exchange, so every rank sees the same count
        self.health.zero_()
        for flat in buckets.flat:
            ops.count_nonfinite(flat, self.health)
        params = model._flat_params()                     # detached views of the nn.Parameters: updated in place
        if self._adam is None:
            quads = []
            for name, g in buckets.grads.items():
                p = params[name]
                st = self.state[name] = dict(step=0, exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p))
                quads.append((p, g, st["exp_avg"], st["exp_avg_sq"]))
            self._adam = ops.AdamTable(quads, model.device)
            self._adam_names = list(buckets.grads)
        self.steps_done += 1
        for st in self.state.values():
            st["step"] = self.steps_done
        norm = clip_and_adam(self._adam, self.steps_done if step_counter is None else step_counter, self.lr, self.betas, self.eps, self.weight_decay,
                             self.health, max_norm=self._max_grad_norm, track=self.track_grad_norm, world=world)
        if norm is not None:
            self._grad_norm = norm
        skipped = self.health[0] > 0                      # device scalar: the buffers below keep their values in a skipped step
        by_dtype = {}
        for name, v in stats.items():                     # BatchNorm running statistics after the three forwards
            if name in params:
                by_dtype.setdefault(params[name].dtype, []).append((params[name], v.to(device=params[name].device, dtype=params[name].dtype)))
        for pairs in by_dtype.values():                   # per dtype: gather, ONE select on the skip word, ONE multi-tensor copy back (96 buffers)
            olds, news = [p for p, _v in pairs], [v for _p, v in pairs]
            sel = torch.where(skipped, torch.cat([p.reshape(-1) for p in olds]), torch.cat([v.reshape(-1) for v in news]))
            torch._foreach_copy_(olds, [c.view(p.shape) for c, p in zip(sel.split([p.numel() for p in olds]), olds)])
        if step_counter is not None:                      # a skipped step does not count (Adam's bias correction, the mask generator's step)
            step_counter.sub_(skipped.to(step_counter.dtype))
        return out, ws

    @contextlib.contextmanager
    def _deferred_range_check(self):
        """Context: `model._engine()` leaves the operand-scale flags of a re-packing unread (no host synchronisation in front of a step);
        `_finish` reads them with the losses."""
        model = self.fwd.model
        model.__dict__["_defer_range_check"] = True
        try:
            yield
        finally:
            model.__dict__["_defer_range_check"] = False

    def _range_flags(self):
        """The device counters of weight operands whose cached power-of-two scale no longer fits (forward packing, backward operands)."""
        pk = self.fwd.model._packed
        return [f for f in (self.fwd.range_flag, pk.range_flag if pk is not None else None) if f is not None]

    def _finish(self, out, ws):
        """Host side of a step: losses, the health word, the range flags (one synchronisation) -> loss dict; raises / skips / re-derives
        scales as `__init__` describes.  Returns (losses, recapture needed)."""
        res = {k: float(v) for k, v in out.items()}
        bad = int(self.health[0])
        stale = any(int(f) != 0 for f in self._range_flags())
        ops.loss_check(ws)
        res["all"] = sum(res.values())
        grad_norm = float(self._grad_norm.norm) if (self._max_grad_norm is not None or self.track_grad_norm) else None
        recapture = False
        if stale:                                         # results of this step are fine (margin of 4x); the NEXT packing takes fresh scales
            self.rescaled += 1
            self.fwd.reset_scales()
            recapture = self._recapture_pending = True
        finite = all(v == v and abs(v) != float("inf") for v in res.values())
        lh = getattr(self, "loss_health", None)
        if lh is not None and int(lh[0]) != 0:            # some rank's loss was non-finite: every rank takes the branch below together
            finite = False
        if bad:                                           # the DEVICE skipped the update (Adam's skip word, the same on every rank: it is counted
            self.steps_done -= 1                          # behind the gradient exchange) — the host only follows that decision
            if grad_norm is not None:                     # how far off the step was: inf / NaN
                res["grad_norm"] = grad_norm
            for st in self.state.values():
                st["step"] = self.steps_done
            msg = (f"training step {self.steps_done + 1}: {bad} non-finite gradient words (losses {res}) — the update was skipped on the device, "
                   f"parameters / Adam moments / BatchNorm buffers are those of the previous step (precision {self.fwd.model.precision!r}, "
                   f"grad_scale {self.fwd.grad_scale:g}: an fp16 plane of the split-fp16 backward overflowed, or the forward met an activation beyond "
                   "|x| < 4094); lower the loss scale (on_nonfinite='skip' halves it) or train with set_precision('fp32')")
            if self.on_nonfinite == "raise":
                raise FloatingPointError(msg)
            self.skipped_steps += 1
            self.fwd.grad_scale *= 0.5
            recapture = self._recapture_pending = True
        elif not finite:
            # a non-finite LOSS whose gradients were all finite: the device applied the update — the health word decides, and
            # it is the only thing all ranks share (losses are rank-local).  Nothing is rolled back, re-scaled or re-captured: host and device
            # step counts stay equal, and no rank starts a warm-up step (with collectives) the others do not run.
            self.nonfinite_loss_steps += 1
            if self.on_nonfinite == "raise":
                raise FloatingPointError(f"training step {self.steps_done}: non-finite loss {res} with finite gradients — the update WAS applied "
                                         "(the device's health word counts gradient words only); optimiser state and step counts are consistent")
        if grad_norm is not None:                         # no loss: it joins the dict behind the decisions above (a skipped step reports inf / NaN)
            res["grad_norm"] = grad_norm
        return res, recapture

    def step(self, batch, iteration=0, dropout_masks=None, random_mask=None, grad_hook=None, speaker_id=None):
        """One optimisation step -> dict of the six losses + "all".  `iteration` is accepted for signature compatibility with the
        reference's train_val_fn (T:132) and unused: the caller computes the mask ratio and passes `random_mask` (T:163-165).
        speaker_id: (B, 1) or (B,) int64 rows of the speaker tables, one per clip (None: zeros, the reference's scripts); a host tensor is
        checked against `speaker_dims` (ValueError)."""
        with self._deferred_range_check():                # the operand-scale flags are read HERE with the losses, not at packing time
            out, ws = self._device_step(batch, dropout_masks, random_mask, grad_hook, speaker_id=speaker_id)
        try:
            res, _ = self._finish(out, ws)
        finally:
            self._parameters_moved()                      # the MFMA operand copies are rebuilt from the updated parameters
            if self._graph is not None:                   # hand-over from the captured step (a ragged last batch runs eagerly): the graph's
                self._step_counter.fill_(self.steps_done) # device-side step counter follows, so a later replay() continues the same count
        return res

    def _parameters_moved(self):
        """`emage_adam_multi` (and a graph replay) update the parameters through raw device pointers: advance their version counters so
        the staleness stamp of `_engine()` sees it (correctness no longer hangs on the call below), and drop the packed set."""
        model = self.fwd.model
        model.bump_versions([p for p in model.parameters() if p.requires_grad])
        model.invalidate_packed()
        self.fwd.parameters_moved()

    # ---- the step as ONE hipGraph -------------------------------------------------------------------------------------------------
    def capture(self, batch, random_mask, dropout_masks=None, prologue=None, speaker_id=None):
        """Capture the whole step — re-packing the MFMA operands from the current parameters, targets, three forwards with their
        backward passes, the dropout masks (drawn on the device from the in-graph step counter unless `dropout_masks` buffers are
        given), Adam, BatchNorm buffers — into one hipGraph over the GIVEN tensors: `batch` and `random_mask` (and `dropout_masks`)
        become the graph's input buffers (refill them in place between replays), the parameters its state.  `replay()` then runs a
        step at device speed instead of the ~10^4 Python-level launches of `step()`.  Both fp32-storage precisions: in f16x3 the
        split-fp16 operand scales are the ones chosen by the warm-up step's packing (a re-packing with known scales is a pure sequence
        of launches).  One eager warm-up step is run and undone.

        prologue: a callable that refills the input buffers ON THE DEVICE (`data.ClipLoader.fill`: `capture(loader.batch, loader.random_mask,
        prologue=loader.fill)`); it runs first inside the captured region, so a replay is "next batch, then the step" and the training loop's
        only host call per step is `replay()`.  It also runs in front of the warm-up step's body; the device tensors it advances (its
        owner's `prologue_state()`: the loader's cursor and iteration) are put back with the optimiser state, so the first replay trains on
        the batch the counters pointed at when `capture` was called.  None (the default): the graph is what it was without the argument.

        speaker_id: a (B, 1) or (B,) int64 DEVICE tensor of per-clip speaker-table rows; it becomes an input buffer of the graph like `batch`
        (refill it in place between replays; `data.ClipLoader.speaker_id` is refilled by the loader's `fill`).  Replays do not read it back:
        the rows are trusted as the store validated them (the kernels clamp).  None: zeros, the graph of a one-speaker step.

        Multi-process runs (round 5): the step is captured WITH its collectives — the four bucket all-reduces (started mid-backward on the
        backend's own stream: they become parallel branches of the graph), SyncBatchNorm's all-gathers and small all-reduces — when the
        backend is "nccl" (= RCCL, whose kernels are stream-capturable), so a multi-rank step is the same graph replay as a single-rank
        one instead of ~10^4 eager launches.  Contract: every rank calls `capture()` (its warm-up step runs the collectives eagerly) and
        then `replay()` the same number of times, with the batch sizes it captured (SyncBatchNorm's global count is the warm-up step's)."""
        fwd, model = self.fwd, self.fwd.model
        if fwd.sync_bn or self._exchanging():
            import torch.distributed as tdist
            backend = tdist.get_backend(self.group) if (tdist.is_available() and tdist.is_initialized()) else None
            if backend is not None and str(backend) != "nccl":
                raise RuntimeError(f"Trainer.capture: the step's collectives can only be captured with the nccl (RCCL) backend, not {backend!r}; "
                                   "use Trainer.step")
        dev = model.device
        for name, t in list(batch.items()) + [("random_mask", random_mask)]:
            if not (torch.is_tensor(t) and t.is_cuda and t.device == dev and t.dtype == torch.float32):
                raise RuntimeError(f"Trainer.capture: {name} must be a float32 tensor on {dev} (it becomes an input buffer of the graph; a host "
                                   "tensor would be copied once at capture time and never again)")
        if speaker_id is not None and not (torch.is_tensor(speaker_id) and speaker_id.is_cuda and speaker_id.device == dev and speaker_id.dtype == torch.int64
                                           and speaker_id.is_contiguous()):
            raise RuntimeError(f"Trainer.capture: speaker_id must be a contiguous int64 tensor on {dev} (it becomes an input buffer of the graph)")
        for fm in (dropout_masks or ()):
            for mk in fm:
                if not (mk.is_cuda and mk.dtype == torch.float32 and mk.is_contiguous()):
                    raise RuntimeError("Trainer.capture: dropout masks must be contiguous fp32 tensors on the device (they are the graph's input buffers)")
        params = model._flat_params()
        saved = {k: v.clone() for k, v in params.items()}
        done = self.steps_done                                         # a RE-capture (new loss scale / operand scales) keeps the optimiser state
        moments = {k: (st["exp_avg"].clone(), st["exp_avg_sq"].clone()) for k, st in self.state.items()}
        owner = getattr(prologue, "__self__", None)
        advanced = list(owner.prologue_state()) if hasattr(owner, "prologue_state") else []
        rewind = [t.clone() for t in advanced]
        self._graph = None
        with self._deferred_range_check():
            if prologue is not None:
                prologue()
            self._device_step(batch, dropout_masks, random_mask, speaker_id=speaker_id)      # warm-up: lazy initialisation inside the library / the allocator, the exchange schedule
        torch.cuda.synchronize(dev)
        for k, v in saved.items():
            params[k].copy_(v)
        for k, st in self.state.items():                               # the moments live OUTSIDE the graph's memory (created by the first warm-up step)
            if k in moments:
                st["exp_avg"].copy_(moments[k][0])
                st["exp_avg_sq"].copy_(moments[k][1])
            else:
                st["exp_avg"].zero_()
                st["exp_avg_sq"].zero_()
            st["step"] = done
        for t, v in zip(advanced, rewind):
            t.copy_(v)
        self.steps_done = done
        self._step_counter = torch.full((1,), done, dtype=torch.int32, device=dev)
        self._graph_inputs = (batch, random_mask, dropout_masks, prologue, speaker_id)       # the graph reads these buffers at every replay: keep them alive
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            model.invalidate_packed()                                  # so that the packing of the current parameters is part of the graph
            fwd.parameters_moved()
            if prologue is not None:
                prologue()
            self._step_counter.add_(1)
            self._graph_out, self._graph_ws = self._device_step(batch, dropout_masks, random_mask, step_counter=self._step_counter, speaker_id=speaker_id)
        self._graph, self._recapture_pending = graph, False
        self._graph_operands = model._packed                           # what the captured launches read (and re-write at every replay)
        model.invalidate_packed()                                      # ... and nobody else: they hold the weights BEFORE the replay's update
        self.steps_done = done
        for st in self.state.values():
            st["step"] = done
        return self

    def replay(self):
        """One captured step on the current contents of the captured input buffers -> the loss dict of `step()`.  A step whose health word
        or operand-scale flags call for it (see `__init__`) is followed by a re-capture over the same input buffers."""
        if self._graph is None:
            raise RuntimeError("Trainer.replay: capture() first")
        if self._recapture_pending:                       # a step that raised behind a scale reset: the graph still carries the old scales
            self.capture(*self._graph_inputs)
        self._graph.replay()
        self.steps_done = int(self._step_counter) + (1 if int(self.health[0]) else 0)      # _finish() takes a skipped step back off
        for st in self.state.values():
            st["step"] = self.steps_done
        model = self.fwd.model
        model._packed = self._graph_operands              # the flags of the graph's own packing
        try:
            res, recapture = self._finish(self._graph_out, self._graph_ws)
        finally:
            self._parameters_moved()                      # a replay moves the parameters through raw pointers: an eval forward behind it
        if recapture:                                     # must re-pack (and never reads the graph's operand set)
            self.capture(*self._graph_inputs)
        return res
