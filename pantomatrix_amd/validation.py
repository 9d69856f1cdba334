"""The validation pass of the training loop on the device — the reference's `train_val_fn(mode="val")` over its test loader
(train_emage_audio.py:130-204, 331-351) — beside `training.Trainer` (the optimisation step) and `data.ClipLoader` (the feed):

    val = validation.Validator(model, vq)
    loader = data.ClipLoader(store, batch, drop_last=False, hold_iteration=True)
    val.capture(loader.batch, loader.random_mask, prologue=loader.fill, n_valid=loader.valid)
    val.reset()
    for _ in range(len(loader)):
        val.replay()
    res = val.result()

One step: `training.targets`, then the three EVAL-mode forwards of the reference (seed mask with audio, random mask with audio, random mask
without audio; BatchNorm on its running statistics, no dropout).  The waveform-only part — both WavEncoders, the audio projection, the
cross-attention K / V — is the same in all three, so it is computed ONCE and handed to them through `EmageAudioModel.forward(_audio_feats=...)`
(the path `inference()` hoists its windows through); the third forward skips the cross-attention stack.  ONE `ops.val_metrics` call (two
launches) then takes the 12 (forward, part) pairs: the six losses and their sum, the arg-max codes of the first forward, and — what the
reference does not log — the top-1 code accuracy of every forward and part, all over the REAL clips of a padded batch (`n_valid`).  The first
forward's codes / latents are routed as `EmageAudioModel._select_codes` does and decoded; `decoded` and `target_rot6d` are the pair the
reference hands to `fgd_evaluator.update`.

Nothing inside a step reads device memory from the host: the per-batch values, the meter sums, the hit / row / batch counters and the sticky
status word live in one accumulator block on the device (`ops.val_accumulators`), which `step()` reads once at its end, `replay()` never, and
`result()` once per pass.  The model is left as found: parameters, buffers and the `training` flag are not touched."""
from __future__ import annotations

import torch

from . import ops, training
from ._lib import EmageKernelError, VAL_ACC_BATCHES, VAL_ACC_HITS, VAL_ACC_METER, VAL_ACC_ROWS, VAL_ACC_STATUS, VAL_LOSSES, VAL_MAX_ENTRIES
from .modeling_emage_audio import _FOLD_WIDTH, _Ctx
from .runtime import PackedGraphs
from .streams import Fork

TAGS = ("seed", "audio", "mask")                          # the three forwards, train_emage_audio.py:156-173
PARTS = ("face", "upper", "hands", "lower")
ENTRY_PARTS = ("upper", "lower", "hands", "face")         # the order get_rec_loss / get_cls_loss add the parts in (T:107-128)
LOSS_KEYS = tuple(f"{kind}_{tag}" for tag in TAGS for kind in ("rec", "cls")) + ("all",)
ENTRIES = tuple((f, p) for f in range(len(TAGS)) for p in ENTRY_PARTS)          # entry e of the kernel's table -> (forward, part)


class Validator:
    """See the module docstring.  `step(batch, random_mask, n_valid=None, speaker_id=None)` runs one batch eagerly and returns its seven losses and twelve
    `acc_<tag>_<part>` as floats; `capture(...)` + `replay()` run it as one hipGraph; `reset()` / `result()` frame a pass over the loader.
    `decoded` / `target_rot6d` ((B, T, 330) static buffers) hold the last step's decoded prediction and its ground truth;
    `codes[tag][part]` ((B, T) int64) every forward's arg-max codes — the decode takes those of the first.  on_decoded(pred, gt): called at
    the end of every EAGER step with those two buffers (the first n_valid clips when n_valid was given as an int).  The frozen VQ models'
    operand sets are packed by the warm-up step of `capture` and read by the graph as they are."""

    def __init__(self, model, vq, on_decoded=None):
        if model.precision == "bf16":
            raise ValueError("the validation step compares with fp32 targets: run it in the fp32-storage precisions (f16x3 / fp32)")
        self.model, self.vq, self.on_decoded = model, vq, on_decoded
        self.acc = ops.val_accumulators(model.device)
        self.decoded, self.target_rot6d, self.codes = None, None, {}
        self._ws, self._full, self._frames = None, {}, None
        self._graph, self._graph_inputs, self._recapture_pending = None, None, False      # _graph: a `runtime.PackedGraphs`

    # ---- one step, device side --------------------------------------------------------------------------------------------------------
    def _n_valid(self, n_valid, bs, dev):
        if n_valid is None or not torch.is_tensor(n_valid):
            n = bs if n_valid is None else int(n_valid)
            if not 0 <= n <= bs:
                raise ValueError(f"Validator: n_valid {n} outside [0, {bs}]")
            if n not in self._full:
                self._full[n] = torch.full((1,), n, dtype=torch.int32, device=dev)
            return self._full[n]
        if n_valid.dtype != torch.int32 or n_valid.numel() != 1 or n_valid.device != dev:
            raise ValueError("Validator: n_valid as a tensor is one int32 on the model's device (data.ClipLoader.valid)")
        return n_valid

    def _static(self, name, like):
        buf = getattr(self, name)
        if buf is None or buf.shape != like.shape or buf.device != like.device:
            if training._capturing():
                raise RuntimeError("Validator: the output buffers are allocated by the warm-up step, not inside a capture")
            buf = torch.empty(tuple(like.shape), dtype=like.dtype, device=like.device)
            setattr(self, name, buf)
        buf.copy_(like)
        return buf

    def _device_step(self, batch, random_mask, n_valid, speaker_id=None):
        model, vq = self.model, self.vq
        cfg = model.config
        was_training = model.training
        if was_training:                                    # the eval forward: running statistics, no dropout, the fused kernels of eval mode
            model.train(False)
        try:
            index, latent, masked_motion = training.targets(vq, batch["motion"], batch["expressions"], batch["trans"], batch["foot_contact"])
            bs, t = masked_motion.shape[:2]
            dev = masked_motion.device
            m = bs * t
            self._frames = t
            n_valid = self._n_valid(n_valid, bs, dev)
            speaker_id = training.speaker_ids(speaker_id, bs, dev, cfg.speaker_dims)      # None: zeros (T:146); the padding clips of a short batch carry the id of the clip they repeat
            seed_mask = torch.ones_like(masked_motion)
            seed_mask[:, :cfg.seed_frames] = 0
            audio = batch["audio"].to(device=dev, dtype=torch.float32)
            if audio.stride(1) != 1:
                audio = audio.contiguous()
            random_mask = random_mask.to(device=dev, dtype=torch.float32)
            # what depends on the waveform only, once for the three forwards (in eval mode it is the same three times)
            cx = _Ctx(model._engine(), model.h2_residual, model.fold_layernorm and cfg.hidden_size == _FOLD_WIDTH)
            with Fork(dev, 3, model.concurrent) as fk:
                feats = model._audio_features(cx, audio, bs, t, True, fk, 1, 2)
            tables = model._speaker_tables(cx, speaker_id, bs, t)
            some = self.codes.get(TAGS[0], {}).get(PARTS[0])
            if some is None or some.shape != (bs, t) or some.device != dev:
                if training._capturing():
                    raise RuntimeError("Validator: the code buffers are allocated by the warm-up step, not inside a capture")
                self.codes = {tag: {p: torch.zeros(bs, t, dtype=torch.int64, device=dev) for p in PARTS} for tag in TAGS}
            weights = {p: (getattr(cfg, "l" + p[0]), getattr(cfg, "c" + p[0])) for p in PARTS}
            entries, first = [], None
            for f, (mask, use_audio) in enumerate(((seed_mask, True), (random_mask, True), (random_mask, False))):
                out = model(audio, speaker_id, masked_motion, mask, use_audio=use_audio, _audio_feats=feats, _tables=tables)
                first = out if f == 0 else first
                for p in ENTRY_PARTS:
                    entries.append(dict(rec=out[f"rec_{p}"].reshape(m, -1), latent=latent[p].reshape(m, -1), logits=out[f"cls_{p}"].reshape(m, -1),
                                        index=index[p].reshape(-1).contiguous(), pred=self.codes[TAGS[f]][p],
                                        l_w=weights[p][0], c_w=weights[p][1], tag=f))
            assert len(entries) == len(ENTRIES) <= VAL_MAX_ENTRIES
            self._ws = ops.val_metrics(entries, t, n_valid, self.acc, self._ws)
            # the first forward's codes / latents -> the decoded motion (T:186-203), routed as `_select_codes` does
            kw = {}
            for p, route in model._routes().items():
                kw[f"{p}_latent"] = first[f"rec_{p}"] if route == "lat" else None
                kw[f"{p}_index"] = self.codes[TAGS[0]][p] if route == "cls" else None
            dec = vq.decode(**kw)["all_motion4inference"]
            self._static("decoded", dec[:, :, :-7])
            self._static("target_rot6d", masked_motion[:, :, :dec.shape[2] - 7])
        finally:
            if was_training:
                model.train(True)

    def _deferred_range_check(self):
        """Context: a re-packing of the eval operand set inside the step leaves its operand-scale flag unread (no host synchronisation in
        the middle of a step); `_check_scales` reads it behind the step."""
        import contextlib
        model = self.model

        @contextlib.contextmanager
        def cm():
            saved = model.__dict__.get("_defer_range_check", False)
            model.__dict__["_defer_range_check"] = True
            try:
                yield
            finally:
                model.__dict__["_defer_range_check"] = saved
        return cm()

    def _stale_scales(self, flag_value):
        """A weight left the range its cached power-of-two operand scale was chosen for (margin: a factor of 4, so the step's numbers
        stand): the next packing chooses the scales afresh, a captured graph is captured again."""
        if flag_value:
            self.model.invalidate_packed(reset_scales=True)
            self._recapture_pending = self._graph is not None
        return bool(flag_value)

    # ---- eager ----------------------------------------------------------------------------------------------------------------------
    def step(self, batch, random_mask, n_valid=None, speaker_id=None):
        """One validation batch, eagerly -> dict of the seven losses (`rec_seed` ... `all`) and `acc_<tag>_<part>` of THIS batch; the meter
        and the counters advance.  n_valid: the real clips of a padded batch — None (all), an int, or one int32 on the device.
        speaker_id: (B, 1) or (B,) int64 rows of the speaker tables, one per clip, read by the three forwards and the shared speaker
        tables (None: zeros); a host tensor is checked against `speaker_dims` (ValueError)."""
        packed_before = self.model._packed
        with self._deferred_range_check():
            self._device_step(batch, random_mask, n_valid, speaker_id)
        r = ops.val_read(self.acc)                           # the step's ONE device-to-host copy
        pk = self.model._packed
        if pk is not None and pk is not packed_before and pk.range_flag is not None:      # a re-packing happened inside the step
            self._stale_scales(int(pk.range_flag))
        if r["status"]:
            raise EmageKernelError("val_metrics: class index out of range (status word set; `reset()` clears it)")
        out = dict(zip(LOSS_KEYS, r["last"]))
        rows = r["last_rows"]
        for e, (f, p) in enumerate(ENTRIES):
            out[f"acc_{TAGS[f]}_{p}"] = r["last_hits"][e] / rows if rows else float("nan")
        if self.on_decoded is not None:
            n = self.decoded.shape[0] if (n_valid is None or torch.is_tensor(n_valid)) else int(n_valid)
            self.on_decoded(self.decoded[:n], self.target_rot6d[:n])
        return out

    # ---- the step as ONE hipGraph ---------------------------------------------------------------------------------------------------
    def capture(self, batch, random_mask, prologue=None, n_valid=None, speaker_id=None):
        """Capture the step — targets, the shared WavEncoder pass, the three forwards, `val_metrics`, the decode — into one hipGraph over the
        given tensors (`batch`, `random_mask`, `n_valid`: refill them in place between replays), and the packing of the eval operand set from
        the CURRENT parameters into a second one, as `Trainer.capture` packs inside its graph: a `replay()` after a training step validates
        the updated parameters, with the operand scales chosen when `capture` ran (checked on the device; `result()` reads the flag and
        schedules a re-capture), and nothing is read back.  prologue: a callable that refills the inputs on the device (`ClipLoader.fill`);
        it runs first inside the step's graph, and the device state it advances (`prologue_state()`) is put back behind the warm-up step,
        as are the accumulators.  speaker_id: None (zeros) or a contiguous int64 DEVICE tensor, (B, 1) or (B,) — a graph input like `batch`
        (`data.ClipLoader.speaker_id`, which the loader's `fill` rewrites)."""
        model = self.model
        dev = model.device
        for name, t in list(batch.items()) + [("random_mask", random_mask)]:
            if not (torch.is_tensor(t) and t.is_cuda and t.device == dev and t.dtype == torch.float32):
                raise RuntimeError(f"Validator.capture: {name} must be a float32 tensor on {dev} (it becomes an input buffer of the graph)")
        if n_valid is not None and not torch.is_tensor(n_valid):
            raise RuntimeError("Validator.capture: n_valid must be None or an int32 device tensor (a graph input)")
        if speaker_id is not None and not (torch.is_tensor(speaker_id) and speaker_id.is_cuda and speaker_id.device == dev and speaker_id.dtype == torch.int64
                                           and speaker_id.is_contiguous()):
            raise RuntimeError(f"Validator.capture: speaker_id must be a contiguous int64 tensor on {dev} (it becomes an input buffer of the graph)")
        owner = getattr(prologue, "__self__", None)
        advanced = list(owner.prologue_state()) if hasattr(owner, "prologue_state") else []
        rewind = [t.clone() for t in advanced] + [self.acc.clone()]
        self._graph = None
        with self._deferred_range_check():
            if prologue is not None:
                prologue()
            self._device_step(batch, random_mask, n_valid, speaker_id)      # warm-up: lazy initialisation, the static buffers, the operand scales
        torch.cuda.synchronize(dev)
        for t, v in zip(advanced + [self.acc], rewind):
            t.copy_(v)
        self._graph_inputs = (batch, random_mask, prologue, n_valid, speaker_id)
        # two graphs over one memory pool (`runtime.PackedGraphs`): the PACKING of the eval operand set from the parameters as they stand
        # when it is replayed, and the step over that set.  Inside a validation pass the parameters stand still, so `replay()` runs the
        # packing only when the model's version stamp has moved (a training step since: `Trainer` advances the counters) — 3.5 ms of a
        # 19 ms replay at 56 clips
        def body():
            if prologue is not None:
                prologue()
            self._device_step(batch, random_mask, n_valid, speaker_id)
        self._graph, self._recapture_pending = PackedGraphs(model, self.vq, body, "Validator.capture: the step"), False
        return self

    def replay(self, repack=None):
        """One captured step on the current contents of the captured input buffers.  Reads nothing back.  repack: None — the operand set
        is packed again when a parameter or buffer of the model has changed since the last replay (the version stamp `_engine()` itself
        goes by); True / False force or suppress it."""
        if self._graph is None:
            raise RuntimeError("Validator.replay: capture() first")
        if self._recapture_pending:
            self.capture(*self._graph_inputs)
        self._graph.replay(repack)

    # ---- a pass ---------------------------------------------------------------------------------------------------------------------
    def reset(self):
        """Zero the meter, the counters and the status word (stream-ordered: a fill on the device, no synchronisation)."""
        self.acc.zero_()

    def result(self, group=None):
        """The pass so far, with ONE device-to-host copy: the reference's meter means `meter[k] / batches` (every batch weighs the same,
        a short last one included: log_train_val, T:504-516), `acc_<tag>_<part>` = hits / rows, `batches` and `clips`.  group (or an
        initialised default process group): the meter sums, batches, hits and rows are summed over the ranks first, in one all-reduce.
        Raises if a class index outside its codebook was met since `reset()`."""
        from . import dist as pdist
        ints = self.acc.view(torch.int64)
        pieces = [self.acc[VAL_ACC_METER:VAL_ACC_METER + VAL_LOSSES], ints[VAL_ACC_HITS:VAL_ACC_STATUS + 1].to(torch.float64)]      # exact below 2^53
        total = pdist.sum_over_group([torch.cat(pieces)], group=group)[0]
        flag = self._graph.operands[0].range_flag if self._graph is not None else None
        host = torch.cat([total, flag.reshape(-1)[:1].to(torch.float64)] if flag is not None else [total]).cpu()
        if flag is not None:
            self._stale_scales(int(host[-1]))
        meter = host[:VAL_LOSSES].tolist()
        counts = [int(v) for v in host[VAL_LOSSES:VAL_LOSSES + VAL_ACC_STATUS + 1 - VAL_ACC_HITS].tolist()]
        hits, rows = counts[:VAL_MAX_ENTRIES], counts[VAL_ACC_ROWS - VAL_ACC_HITS]
        batches, status = counts[VAL_ACC_BATCHES - VAL_ACC_HITS], counts[VAL_ACC_STATUS - VAL_ACC_HITS]
        if status:
            raise EmageKernelError("val_metrics: class index out of range (status word set; `reset()` clears it)")
        if batches == 0:
            raise RuntimeError("Validator.result: no batch since reset()")
        out = {k: v / batches for k, v in zip(LOSS_KEYS, meter)}
        for e, (f, p) in enumerate(ENTRIES):
            out[f"acc_{TAGS[f]}_{p}"] = hits[e] / rows
        out["batches"], out["clips"] = batches, rows // self._frames if self._frames else 0
        return out
