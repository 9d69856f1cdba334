"""MI355X-native EMAGE model classes — the host side of the drop-in boundary.

Same public surface as /root/reference/models/emage_audio/modeling_emage_audio.py:

* ``EmageVAEConv`` (M:19-32), ``EmageVQVAEConv`` (M:34-70), ``EmageVQModel`` (M:72-205),
  ``EmageAudioModel`` with ``forward`` (M:265-341) and ``inference`` (M:343-490);
* same state-dict keys (``pantomatrix_amd/spec.py``), same (B,T,C) fp32 tensors at the API,
  int64 indices, float 0/1 masks with 1 = masked.

Nothing here computes on the CPU: every arithmetic op is a launch into libemage_hip.so
(``pantomatrix_amd/ops.py`` -> ``include/emage_hip.h``); torch supplies device memory, the
current HIP stream and small index/shape plumbing.  There is no fallback path — tensors must be on
a ROCm device and the library must be built, otherwise calls raise.

Precision: ``set_precision("f16x3")`` (default; fp32 storage, every product as three split-fp16 MFMAs:
fp32-grade, reproduces the reference's VQ code indices), ``set_precision("fp32")`` (exact-fp32 MFMA
everywhere) or ``set_precision("bf16")`` (bf16 MFMA operands, fp32 accumulate / residual stream /
LayerNorm / softmax / arg-min: fastest, not index-exact).
"""
from __future__ import annotations

import contextlib
import json
import os
from typing import NamedTuple

import torch

from . import ops, spec, synthetic, windows
from .streams import Fork
from ._lib import BF16, F32, F16X3, H2
from .configuration_emage_audio import EmageAudioConfig, EmageVAEConvConfig, EmageVQVAEConvConfig

OUT_KEYS = ("rec_face", "rec_upper", "rec_hands", "rec_lower", "cls_face", "cls_upper", "cls_hands", "cls_lower")
_PRECISIONS = {"bf16": BF16, "fp32": F32, "f16x3": F16X3}
_PRECISION_NAMES = {v: k for k, v in _PRECISIONS.items()}
_WAV_TAPS = spec.WAV_KERNEL


_NARROW = 32          # WavEncoder width of DisCo / CaMN's first blocks: half a 64-channel operand row (see _Packed.conv_pairs)


_FOLD_WIDTH = 768        # the LayerNorm fold's row statistics are 24 partials of 32 columns (include/emage_hip.h: ln_np == 24): hidden_size 768 only


def _rup(x, m=64):
    return (x + m - 1) // m * m


# ======================================================================================
# parameter container with the HuggingFace-style persistence the reference gets from
# transformers.PreTrainedModel (config.json + model.safetensors / pytorch_model.bin)
# ======================================================================================
class _ParamNode(torch.nn.Module):
    """A bare node of the module tree: it only holds the parameters / buffers registered under the reference's names."""


_BUFFER_ROLES = ("bn_mean", "bn_var", "bn_count", "ppe")       # BatchNorm running statistics, the positional table


class _EmageModule(torch.nn.Module):
    """torch.nn.Module whose parameter tree reproduces the reference module's names (so `state_dict()`,
    `load_state_dict()`, `named_parameters()`, `.to()`, hooks, wrapping all behave as for the reference classes), and
    whose forward is a sequence of libemage_hip.so launches over lazily packed copies of those parameters.  The packed
    copies are dropped whenever the parameters may have changed (`load_state_dict`, `.to()` / `.cuda()` / dtype casts,
    `set_precision`, or an explicit `invalidate_packed()` after in-place edits)."""
    config_class = None
    _spec_fn = None

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.cfg = config                      # the reference exposes `.cfg` (M:214, test_emage_audio.py:34-42)
        self._dt = F16X3                       # the parity-green mode is the default; see set_precision
        self._packed = None
        self.concurrent = True                 # issue independent launch chains on side streams (streams.py)
        self.hoist_audio = True                # inference(): waveform-only features of all full windows in one pass
        self.seed_only_decode = True           # inference(): per-window decode covers only the frames that feed the seed
        self.health_counter = None             # optional int32 device counter of non-finite logits / latents met by infer_codes (runtime.ClipRunner)
        self.health_pending = None             # ... or a list that collects those tensors instead (`collect_health()`): the caller counts them in one launch
        self.slab_convs = True                 # WavEncoder: LDS-resident-slab convolutions + fused block 0 (A/B switch; same bits)
        self.h2_residual = True                # EMAGE_H2 mode: LayerNorm writes ONE output, the H2 image, and the sub-layers read their residual from
                                               # it ((hi + lo) / 16: 2^-22 relative); False = a float32 twin beside every H2 image (round 3's default:
                                               # 25 instead of 12.6 MB per LayerNorm at 64 clips).  Parity-green on every golden in both forms
        self.fold_layernorm = True             # EMAGE_H2 mode with H2 residuals: the interior LayerNorms of the post-norm transformer layers are
                                               # FOLDED into the contractions around them (LN(s) W^T + b = rstd (s W'^T - mu c) + b': 41 of the 47
                                               # LayerNorm launches of a window disappear; include/emage_hip.h: emage_gemm_problem); False = every
                                               # LayerNorm is a launch (round 5's form).  Parity-green on every golden in both forms
        self.split_acts = True                 # f16x3 precision: activations that feed a contraction are stored PRE-SPLIT (EMAGE_H2,
                                               # csrc/h2.h) by their producers; False = float32 activations split inside every GEMM
        self.activation_shift = 0              # EMAGE_H2 mode: activation images hold x * 2^(4 - shift) (include/emage_hip.h EMAGE_H2_SHIFT): 0 = the
                                               # parity-green default (|x| < 4094); a checkpoint with larger activations runs with shift k
                                               # (|x| < 4094 * 2^k) instead of leaving the split-fp16 path — `set_activation_shift`,
                                               # `runtime.ClipRunner(on_overflow="rescale")`, `runtime.calibrate_activation_shift`
        self.group_gemms = True                # part-wise stacks (VQ part decoders, refinement layers + heads, ...) walk in lock step and
                                               # their contractions share launches (ops.lockstep / emage_gemm_grouped); False = one stream
                                               # lane per chain, one launch per contraction (the round-3 form; same bits)
        self.fuse_self_attention = True        # EMAGE_H2 eval forward, 64-frame windows of enough clips to fill the GPU: each self-attention site's qkv
                                               # projection and attention run as ONE launch (ops.qkv_attention: q / k / v never leave the chip);
                                               # False = the two launches (same bits)
        self.fuse_cross_attention = True       # the same for the cross-attention sites: the q projection and the attention on the layer's memory
                                               # K / V^T run as ONE launch (ops.q_attention: q never leaves the chip); False = the two launches (same bits)
        self.compose_memory = True             # EMAGE_H2 eval forward (ignored elsewhere): each decoder stack's memory projection (`audio_body_motion_proj`,
                                               # `audio_face_motion_proj`) is COMPOSED with the stack's K / V projections at packing time (`_Packed._compose`):
                                               # the K / V contraction runs on the 256 / 512 feature columns and the projected memory is never computed;
                                               # False = the two Linear layers one after the other (re-associates the arithmetic: parity-green on every golden)
        self.fuse_memory_kv = True             # ... and each stack cross-attention site that `fuse_cross_attention` fuses computes its K / V^T itself from
                                               # the feature image (ops.qm_attention: no K / V^T tensor); False = one composed K / V launch per stack (same bits)
        self.group_face_body = False           # forward(): the 4 face decoder layers walk in lock step with the first 4 audio cross-attention
                                               # layers of the body (same shapes, different weights: 6 contractions per layer pair share
                                               # launches) instead of running on two stream lanes; same bits (A/B switch)
        self._templates = {}                   # cached default motion / mask of inference() per (batch, length, device)
        self._spec = type(self)._spec_fn(config)
        init = synthetic.state_dict_from_spec(self._spec, seed=int(getattr(config, "init_seed", 0)), cfg=config,
                                              prefix=type(self).__name__ + "/")
        for name, (_shape, role) in self._spec.items():
            node, parts = self, name.split(".")
            for part in parts[:-1]:
                if part not in node._modules:
                    node.add_module(part, _ParamNode())
                node = node._modules[part]
            if role in _BUFFER_ROLES:
                node.register_buffer(parts[-1], init[name])
            else:
                node.register_parameter(parts[-1], torch.nn.Parameter(init[name], requires_grad=init[name].is_floating_point()))
        self.eval()

    # ---- nn.Module surface ------------------------------------------------------------
    @property
    def device(self):
        return next(self.parameters()).device

    def state_dict(self, *args, **kwargs):
        """The reference's keys in the reference's order (`pantomatrix_amd/spec.py`)."""
        sd = super().state_dict(*args, **kwargs)
        if args or kwargs.get("destination") is not None:      # called by a parent module: it owns the destination dict
            return sd
        prefix = kwargs.get("prefix", "")
        ordered = type(sd)((prefix + k, sd[prefix + k]) for k in self._spec if prefix + k in sd)
        for k, v in sd.items():
            ordered.setdefault(k, v)
        if hasattr(sd, "_metadata"):
            ordered._metadata = sd._metadata
        return ordered

    def load_state_dict(self, state_dict, strict=True, assign=False):
        out = super().load_state_dict(state_dict, strict=strict, assign=assign)
        self.__dict__["_scale_caches"] = {}      # new weights: the split-fp16 operand scales are chosen afresh
        self.invalidate_packed()
        return out

    def _apply(self, fn, recurse=True):         # .to() / .cuda() / .cpu() / .float() ... all funnel through here
        out = super()._apply(fn, recurse)
        self.invalidate_packed()
        return out

    def invalidate_packed(self, reset_scales=False):
        """Drop the packed operand copies; the next forward re-packs from the current parameters.  reset_scales: also forget the
        power-of-two operand scales of the split-fp16 modes (chosen at the first packing and kept across re-packings so that a training
        step re-packs without a host read-back) — for weights REPLACED other than through this module's `load_state_dict`."""
        self._packed = None
        self._templates = {}
        self.__dict__.pop("_version_slots", None)       # parameters / buffers / submodules registered since the last stamp are tracked from the next one on
        if reset_scales:
            self.__dict__["_scale_caches"] = {}
        return self

    def _version_stamp(self):
        """Identity and in-place version counter of every parameter and buffer: what `_engine()` compares with the stamp taken at packing
        time, so an optimiser step, a BatchNorm-buffer update of a train-mode forward, `p.data.copy_()`, a parent module's
        `load_state_dict` ... are all followed by a re-pack — in eval mode too (train, `optimizer.step()`, `model.eval();
        model(...)`).  The stamp reads the CURRENT objects out of each owning module's `_parameters` / `_buffers` dict (a
        tensor REPLACED after packing — `module.weight = nn.Parameter(...)`, a re-registered buffer — has a new identity and re-packs too);
        only the list of (dict, key) slots is cached (the module tree is fixed at construction): ~500 dict reads, no `state_dict()` walk."""
        slots = self.__dict__.get("_version_slots")
        if slots is None:
            slots = []
            for mod in self.modules():
                slots.extend((mod._parameters, k) for k in mod._parameters)
                slots.extend((mod._buffers, k) for k in mod._buffers if k not in mod._non_persistent_buffers_set)
            self.__dict__["_version_slots"] = slots
        stamp = []
        for d, k in slots:
            t = d.get(k)
            stamp.append((id(t), t._version) if t is not None else (0, 0))
        return tuple(stamp)

    @staticmethod
    def bump_versions(tensors):
        """Advance the version counters of tensors that were updated through raw device pointers (`emage_adam_multi`, a graph replay): the
        staleness check of `_engine()` then sees the update without anyone having to call `invalidate_packed()`."""
        ts = [t for t in tensors if torch.is_tensor(t)]
        if not ts:
            return
        try:
            torch._C._autograd._unsafe_set_version_counter(ts, [t._version + 1 for t in ts])
        except (TypeError, AttributeError, RuntimeError):       # a torch whose private setter takes one tensor at a time, or has none
            setter = getattr(torch._C._autograd, "_unsafe_set_version_counter", None)
            for t in ts:
                try:
                    setter(t, t._version + 1)
                except Exception:                               # noqa: BLE001 — last resort: an in-place no-op advances the counter
                    with torch.no_grad():
                        t.add_(0)

    _trainable = False       # EmageAudioModel: train() switches forward() to the differentiable train-mode forward

    def train(self, mode=True):
        if mode and not self._trainable:
            raise NotImplementedError(f"{type(self).__name__} has an eval-mode forward only (the reference keeps its VQ-VAEs frozen, "
                                      "train_emage_audio.py:233-245); the trainable class is EmageAudioModel")
        return super().train(mode)

    def set_activation_shift(self, shift: int):
        """See `activation_shift`.  Takes effect at the next forward (the packed weights do not change: their scales are per tensor already);
        a captured graph keeps the shift it was captured with."""
        ops.h2_shifted(shift)                  # validates the range
        self.activation_shift = int(shift)
        return self

    def set_precision(self, precision: str):
        if precision not in _PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_PRECISIONS)}")
        if _PRECISIONS[precision] != self._dt:
            self._dt = _PRECISIONS[precision]
            self._packed = None
        return self

    @property
    def precision(self):
        return _PRECISION_NAMES[self._dt]

    # ---- persistence ---------------------------------------------------------------
    def save_pretrained(self, save_directory):
        from safetensors.torch import save_file
        self.config.save_pretrained(save_directory)
        save_file({k: v.detach().cpu().contiguous() for k, v in self.state_dict().items()},
                  os.path.join(save_directory, "model.safetensors"), metadata={"format": "pt"})

    @classmethod
    def from_pretrained(cls, path, subfolder=None, **_unused):
        """Load a HuggingFace-format directory (config.json + model.safetensors | pytorch_model.bin).  A hub
        repo id is resolved through huggingface_hub when it is not a local directory (needs network)."""
        root = path
        if not os.path.isdir(root):
            from huggingface_hub import snapshot_download
            root = snapshot_download(path)
        d = os.path.join(root, subfolder) if subfolder else root
        with open(os.path.join(d, "config.json")) as f:
            cfg = json.load(f)
        for k in ("model_type", "architectures", "transformers_version", "torch_dtype", "dtype"):
            cfg.pop(k, None)
        model = cls(cls.config_class(**cfg))
        st = os.path.join(d, "model.safetensors")
        if os.path.exists(st):
            from safetensors.torch import load_file
            sd = load_file(st)
        else:
            sd = torch.load(os.path.join(d, "pytorch_model.bin"), map_location="cpu", weights_only=True)
        model.load_state_dict(sd, strict=True)
        return model

    # ---- engine plumbing -------------------------------------------------------------
    _supports_h2 = True      # the class's forward handles EMAGE_H2 activations (the LSTM models keep float32 activations)

    @staticmethod
    def _require_device(dev):
        if dev.type != "cuda":
            raise RuntimeError("the EMAGE model classes run only on an MI355X device: call .to('cuda') first "
                               "(there is no CPU fallback; the CPU oracle lives in oracle/ for tests only)")

    def _engine(self, h2=None, train_only=False):
        """The packed operand set of the current precision.  h2 (f16x3 only): pre-split EMAGE_H2 operands (default: `split_acts`);
        the training forward asks for h2=False (float32 activations, weights in the EMAGE_F16X3 packing) and train_only=True: `_pack` may
        then leave out operands only the eval-mode forward reads (a training step re-packs behind every update); such a set is never
        handed to an eval-mode caller."""
        dev = self.device
        self._require_device(dev)
        want_h2 = self._dt == F16X3 and self._supports_h2 and (self.split_acts if h2 is None else h2)
        dt = H2 if want_h2 else self._dt
        stamp = self._version_stamp()
        compose = bool(self.compose_memory) and dt == H2 and not train_only        # eval sets only: a training forward never reads the composed operands
        if (self._packed is None or self._packed.device != dev or self._packed.dt != dt or self._packed.stamp != stamp
                or (not train_only and (self._packed.train_only or self._packed.compose != compose))):
            capturing = dev.type == "cuda" and torch.cuda.is_current_stream_capturing()
            for attempt in (0, 1):
                # the scale cache is keyed by packing ORDER: a train-only set (fewer operands) keeps its own
                ckey = (str(dev), dt, bool(train_only))
                cache = self.__dict__.setdefault("_scale_caches", {}).setdefault(ckey, {})
                pk = _Packed(self._flat_params(), dev, dt, cache)
                pk.stamp, pk.train_only, pk.compose = stamp, bool(train_only), compose
                self._pack(pk)
                pk.finish_range_check()
                # a weight that left the range its cached power-of-two scale was chosen for (it grew / shrank 4x since the first packing, or
                # was replaced): choose the scales afresh.  Outside a stream capture only (the flag is read on the host); a training step
                # (`training.Trainer`, eager or captured) leaves the flag unread here and reads it with its losses
                if attempt == 0 and not capturing and not self.__dict__.get("_defer_range_check") and pk.range_flag is not None and int(pk.range_flag) != 0:
                    self.__dict__["_scale_caches"].pop(ckey, None)
                    continue
                break
            self._packed = pk
        self._packed.act_shift = int(self.activation_shift)
        return self._packed

    def _flat_params(self):
        """name -> detached tensor, the view of the parameter tree the packer reads."""
        return {k: v.detach() for k, v in super().state_dict(keep_vars=True).items()}

    def _pack(self, pk):
        raise NotImplementedError


# ======================================================================================
# packed weights: MFMA-operand dtype, K-contiguous rows, taps flattened, BatchNorm folded
# ======================================================================================
class _Packed:
    def __init__(self, params, device, dt, scale_cache=None):
        self.p, self.device, self.dt = params, device, dt
        self.act_shift = 0           # the owning module's `activation_shift` at the time the set was handed out (`_engine`): read by `_Ctx`
        # split-fp16 operand scales by packing order: chosen (one read-back of max|w|) at the FIRST packing of a model's weights and kept for
        # every re-packing (after an optimiser step: a pure sequence of launches, capturable); cleared when a state dict is loaded
        self.scale_cache = {} if scale_cache is None else scale_cache
        self._n_operands = 0
        self.stamp = None            # `_EmageModule._version_stamp()` of the parameters this set was packed from
        self.compose = False         # the set holds the composed memory operands (`_EmageModule.compose_memory`; EMAGE_H2 eval sets only)
        self.train_only = False      # packed for the training forward alone (`_engine(train_only=True)`): eval-only operands may be missing
        # int32 device counter of operands packed with a CACHED scale whose max |w * scale| has left [2^10, 2^14) (chosen into
        # [2^12, 2^13): the fp16 hi plane overflows at 2^16); None until such a packing happens
        self.range_flag = None
        self._range_pending = []
        self.wav_dt = F16X3 if dt == H2 else dt      # the WavEncoder keeps float32 activations (slab kernels split in LDS)
        self.tdt = ops.TORCH_DTYPE[dt]
        self.w = {}
        self.origin = {}     # key -> [(weight name, bias name, row slice of that parameter)] in stacking order (training: gradient unpacking)
        # per-column LeakyReLU slope vectors, built once here (before any stream fork can race on them):
        # 0 = ReLU, 0.01 / 0.1 / 0.2 = the reference's LeakyReLU slopes
        self._slopes = {v: torch.full((4096,), v, dtype=torch.float32, device=device) for v in (0.0, 0.01, 0.1, 0.2)}

    def finish_range_check(self):
        """Fold the operands packed with a CACHED scale since the last call into `range_flag` (how many of them have left the band their
        scale was chosen for): called once behind a packing pass."""
        if self._range_pending:
            ws, scales = zip(*self._range_pending)
            self._range_pending = []
            bad = ops.f16_scales_out_of_range(list(ws), list(scales))
            self.range_flag = bad if self.range_flag is None else self.range_flag + bad

    def slope(self, value, n):
        return self._slopes[float(value)][:n]

    def f32(self, name):
        return self.p[name].to(torch.float32).contiguous()

    def _operand(self, w2d, dt=None):
        """(N, K) fp32 with K already padded -> the MFMA operand image of precision `dt` (default: the model's) and its scale."""
        dt = self.dt if dt is None else dt
        if dt in (H2, F16X3):
            key = (dt, self._n_operands, tuple(w2d.shape))
            self._n_operands += 1
            cached = self.scale_cache.get(key)
            img, scale = (ops.split_f16_weights_h2 if dt == H2 else ops.split_f16_weights)(w2d.contiguous(), cached)
            self.scale_cache[key] = scale
            if cached is not None and w2d.numel():
                self._range_pending.append((w2d, scale))          # checked together by `finish_range_check` (a few launches for all of them)
            return img, scale
        out = w2d.to(ops.TORCH_DTYPE[dt]).contiguous()
        return (out.clone() if out.data_ptr() == w2d.data_ptr() else out), 1.0          # never a view of the parameter itself

    def _pack_mat(self, w2d):
        n, k = w2d.shape
        kp = _rup(k)
        if kp != k:
            w2d = torch.nn.functional.pad(w2d, (0, kp - k))
        w, ws = self._operand(w2d)
        return w, kp, ws

    def _fold_norm(self, wcat, bcat, norm):
        """A LayerNorm folded into the Linear that consumes it (include/emage_hip.h: emage_gemm_problem): LN(s) W^T + b =
        rstd (s W'^T - mu c) + b' with W' = W gamma, c[n] = sum_k W'[n][k], b' = W beta + b -> (W', b', c)."""
        g, be = self.p[norm + ".weight"].float(), self.p[norm + ".bias"].float()
        w2 = wcat * g[None, :]
        return w2, (bcat.double() + wcat.double() @ be.double()).float(), w2.double().sum(dim=1).float().contiguous()

    def _compose(self, wcat, bcat, proj):
        """The Linear `proj` in front of this one with nothing between them, composed into it: (a Wp^T + bp) W^T + b = a (W Wp)^T + (W bp + b)
        -> (W Wp, W bp + b), both products in float64 from the float32 parameters and rounded to float32 once."""
        wp, bp = self.p[proj + ".weight"].double(), self.p[proj + ".bias"].double()
        return (wcat.double() @ wp).float().contiguous(), (wcat.double() @ bp + bcat.double()).float().contiguous()

    @staticmethod
    def _stack(ts):
        """torch.cat(ts, 0) — or, when the pieces are consecutive row blocks of ONE contiguous tensor in memory order (the q / k / v blocks of an
        in_proj weight, a single source), the view that covers them: the operand packing reads the parameter itself instead of a copy of it
        (~170 concatenation launches per training step, which re-packs behind every update)."""
        t0 = ts[0]
        if len(ts) == 1:
            return t0
        if all(t.is_contiguous() and t.dtype == t0.dtype and t.shape[1:] == t0.shape[1:] and t.untyped_storage().data_ptr() == t0.untyped_storage().data_ptr() for t in ts):
            if all(b.storage_offset() == a.storage_offset() + a.numel() for a, b in zip(ts, ts[1:])):
                return torch.as_strided(t0, (sum(t.shape[0] for t in ts),) + tuple(t0.shape[1:]), t0.stride(), t0.storage_offset())
        return torch.cat(ts, 0)

    def _bias(self, bs):
        """The stacked bias vector of an entry.  A train-only set (re-packed behind every optimiser step, dropped with it) may read the parameter
        in place; every other set keeps its own copy (an eval-mode set outlives in-place edits until the next stamp check)."""
        if not self.train_only:
            return torch.cat(bs).float().contiguous()
        b = self._stack(bs).float()
        return b if (b.is_contiguous() and b.data_ptr() % 16 == 0) else b.clone()      # the kernels read bias vectors 16 bytes at a time

    def linear(self, key, names, rows=None, fold=None):
        """Stack nn.Linear weights along N (optionally row-slices `rows[i]` of each) -> entry `key`.  fold: the name of the LayerNorm
        whose output is this Linear's operand — the entry then holds the FOLDED operands (`_fold_norm`) and `c`; eval only."""
        ws, bs = [], []
        for i, nm in enumerate(names):
            w, b = self.p[nm + ".weight"], self.p[nm + ".bias"]
            if rows is not None:
                w, b = w[rows[i]], b[rows[i]]
            ws.append(w)
            bs.append(b)
        k_real = ws[0].shape[1]
        wcat = self._stack(ws).float()                                    # one source / adjacent blocks: the operand packing reads the parameter itself
        bcat = self._bias(bs)
        extra = {}
        if fold is not None:
            wcat, bcat, c = self._fold_norm(wcat, bcat, fold)
            extra = dict(c=c, norm=fold)
        w, kp, wsc = self._pack_mat(wcat)
        self.w[key] = dict(w=w, b=bcat, n=wcat.shape[0], cp=kp, taps=1, k_real=k_real, ws=wsc, dt=self.dt, **extra)
        if fold is None:
            self.origin[key] = [(nm + ".weight", nm + ".bias", rows[i] if rows is not None else slice(0, self.p[nm + ".weight"].shape[0]))
                                for i, nm in enumerate(names)]

    def in_proj(self, key, names, parts, fold=None, compose=None):
        """Row blocks of packed in_proj weights: parts e.g. "qkv", "q", "kv"; several layers stack as
        [K_0..K_n | V_0..V_n] so that one GEMM emits every layer's K and V^T (V columns last).  fold: see `linear`.  compose: the name of the
        Linear whose output is this projection's ONLY consumer-side operand — the entry then contracts that Linear's input (`_compose`); eval only."""
        d = self.p[names[0] + ".in_proj_weight"].shape[1]
        sl = {"q": slice(0, d), "k": slice(d, 2 * d), "v": slice(2 * d, 3 * d)}
        ws, bs = [], []
        origin = []
        for part in parts:
            for nm in names:
                ws.append(self.p[nm + ".in_proj_weight"][sl[part]])
                bs.append(self.p[nm + ".in_proj_bias"][sl[part]])
                origin.append((nm + ".in_proj_weight", nm + ".in_proj_bias", sl[part]))
        k_real = ws[0].shape[1]
        wcat = self._stack(ws).float()
        bcat = self._bias(bs)
        extra = {}
        if compose is not None:
            assert fold is None
            wcat, bcat = self._compose(wcat, bcat, compose)
            k_real = wcat.shape[1]
        elif fold is not None:
            wcat, bcat, c = self._fold_norm(wcat, bcat, fold)
            extra = dict(c=c, norm=fold)
        else:
            self.origin[key] = origin
        w, kp, wsc = self._pack_mat(wcat)
        self.w[key] = dict(w=w, b=bcat, n=wcat.shape[0], cp=kp, taps=1, k_real=k_real, ws=wsc, dt=self.dt, **extra)

    def folded(self, cname, bn=None):
        """Raw Conv1d (weight (Cout,Cin,k), bias) with an eval-mode BatchNorm1d folded in:
        W' = W*g/sqrt(var+eps), b' = (b-mean)*g/sqrt(var+eps)+beta (eps 1e-5)."""
        w, b = self.p[cname + ".weight"].float(), self.p[cname + ".bias"].float()
        if bn is not None:
            s = self.p[bn + ".weight"].float() / torch.sqrt(self.p[bn + ".running_var"].float() + 1e-5)
            w = w * s[:, None, None]
            b = (b - self.p[bn + ".running_mean"].float()) * s + self.p[bn + ".bias"].float()
        return w, b

    def conv(self, key, name, fold_bn=None, extra=None, dt=None):
        """Conv1d weight (Cout,Cin,k) -> (Cout, k*Cp), taps major, channels zero-padded to Cp; `extra`
        = (conv, bn) stacks a second conv (the downsample shortcut) along Cout.  dt: operand packing (default: the model's)."""
        dt = self.dt if dt is None else dt
        w, b = self.folded(name, fold_bn)
        if extra is not None:
            w2, b2 = self.folded(*extra)
            w, b = torch.cat([w, w2], 0), torch.cat([b, b2])
        cout, cin, k = w.shape
        cp = _rup(cin)
        w = w.permute(0, 2, 1)                                   # (Cout, k, Cin)
        if cp != cin:
            w = torch.nn.functional.pad(w, (0, cp - cin))
        wp, wsc = self._operand(w.reshape(cout, k * cp), dt)
        self.w[key] = dict(w=wp, b=b.contiguous(), n=cout, cp=cp, taps=k, k_real=k * cin, ws=wsc, dt=dt)

    def conv_pairs(self, key, w, b, slope, stride, pad):
        """A Conv1d over NARROW rows (Cin = 32) as a convolution over PAIRS of positions: the (L, 32) activation rows of a
        sequence are, in memory, (L/2, 64) rows [x[2p] | x[2p+1]], so a 64-channel kernel (slab / implicit GEMM) runs it
        without the 2x zero padding of K (and, for stride 1, of N: the output pair [y[2p] | y[2p+1]] is one 64-wide row).
          stride 1:  out pair p, half ho  <-  in pair p+q, half hi  through tap 2q + hi - ho + pad   (q = -4..4 for k = 15)
          stride 2s: out row p            <-  in pair s*p + q, half hi through tap 2q + hi           (pad must be 0)
        w (Cout, Cin, k) / b / slope are the folded conv; entry: w (N, taps_p * 64) packed, n, taps, pad, stride in pair units."""
        cout, cin, k = w.shape
        assert cin * 2 == 64
        if stride == 1:
            qs = sorted({q for q in range(-k, k + 1) for hi in (0, 1) for ho in (0, 1) if 0 <= 2 * q + hi - ho + pad < k})
            wp = torch.zeros(2, cout, len(qs), 2, cin, dtype=torch.float32, device=w.device)
            for ho in (0, 1):
                for hi in (0, 1):
                    for j, q in enumerate(qs):
                        tau = 2 * q + hi - ho + pad
                        if 0 <= tau < k:
                            wp[ho, :, j, hi, :] = w[:, :, tau]
            wp = wp.reshape(2 * cout, len(qs) * 2 * cin)
            b, slope = torch.cat([b, b]), torch.cat([slope, slope])
            ent = dict(n=2 * cout, taps=len(qs), pad=-qs[0], stride=1)
        else:
            assert stride % 2 == 0 and pad == 0
            nq = (k + 1) // 2
            wp = torch.zeros(cout, nq, 2, cin, dtype=torch.float32, device=w.device)
            for q in range(nq):
                for hi in (0, 1):
                    if 2 * q + hi < k:
                        wp[:, q, hi, :] = w[:, :, 2 * q + hi]
            wp = wp.reshape(cout, nq * 2 * cin)
            ent = dict(n=cout, taps=nq, pad=0, stride=stride // 2)
        wpk, wsc = self._operand(wp, self.wav_dt)
        self.w[key] = dict(w=wpk, b=b.float().contiguous(), slope=slope.float().contiguous(), cp=2 * cin, k_real=k * cin, ws=wsc, dt=self.wav_dt, **ent)

    def norm(self, key, name):
        self.w[key] = dict(g=self.f32(name + ".weight"), b=self.f32(name + ".bias"))


# ======================================================================================
# kernel-call helpers shared by the model classes
# ======================================================================================
class _Ctx:
    """One forward's launch context: packed weights + dtype + allocation helpers."""

    def __init__(self, pk: _Packed, h2_residual=False, fold_ln=False):
        # h2_residual (EMAGE_H2 mode): LayerNorm writes ONLY the H2 image and the sub-layer epilogues read the residual from it
        # ((hi + lo) / 16: 2^-22 relative to the float32 value) instead of from a float32 twin: one 12.6 MB store less per norm
        self.h2res = bool(h2_residual) and pk.dt == H2
        # dt: storage / elementwise-kernel type of activations; gdt: emage_gemm's operand mode (F16X3 = float32 storage,
        # split-f16 MFMA; equal to dt otherwise)
        self.pk, self.gdt, self.tdt, self.dev = pk, pk.dt, pk.tdt, pk.device
        self.h2 = pk.dt == H2                   # activations that feed a contraction are EMAGE_H2 images (float32-sized elements)
        self.dt = F32 if pk.dt == F16X3 else pk.dt
        # h2dt: the dtype code of ACTIVATION images — EMAGE_H2 carrying the model's activation shift (`_EmageModule.activation_shift`,
        # include/emage_hip.h EMAGE_H2_SHIFT): every launch that writes or reads one takes it; 0 (the default) is plain EMAGE_H2
        self.h2dt = ops.h2_shifted(pk.act_shift if self.h2 else 0)
        if self.h2:
            self.gdt = self.dt = self.h2dt
        # WavEncoder: float32 activations in both split-f16 forms (its slab kernels split once per block in LDS)
        self.wgdt = pk.wav_dt
        self.wdt = F32 if pk.wav_dt == F16X3 else pk.wav_dt
        # fold_ln (EMAGE_H2 with H2 residuals; `model.fold_layernorm`): interior LayerNorms of the post-norm layers are FOLDED into the
        # contractions around them (include/emage_hip.h: emage_gemm_problem) — no LayerNorm launch, no normalised tensor
        self.fold_ln = bool(fold_ln) and self.h2res
        # compose (`model.compose_memory`): the set holds the stacks' composed memory K / V operands — the forward contracts the feature images
        self.compose = bool(pk.compose) and self.h2

    def lo(self, m, n):
        return torch.empty(m, n, dtype=self.tdt, device=self.dev)

    def f32(self, m, n):
        return torch.empty(m, n, dtype=torch.float32, device=self.dev)

    def gemm(self, a, key, *, slope=None, res=None, res_first=False, out=None, out_f32=None, want="lo", n_store=0,
             out_t=None, t_col0=0, t_rows=0, conv=None, m=None, dt=None, w=None, res_h2=False, ln=None, res_ln=None, stats_out=None):
        """Run one contraction.  want: "lo", "f32", "both" allocate the outputs when not passed in.
        conv = (stride, pad, lin, lout) turns it into the implicit-GEMM Conv1d with the entry's tap count.
        The operand mode is the weight entry's packing (EMAGE_H2 entries take an H2 image `a` and write H2 `lo` outputs;
        res_h2: the residual is an H2 image too, else float32)."""
        e = w if w is not None else self.pk.w[key]
        dt = e.get("dt", self.gdt) if dt is None else dt
        if dt == H2:
            dt = self.h2dt
        h2 = dt & 0xff == H2
        m = a.shape[0] if m is None else m
        n = e["n"]
        if out is None and out_t is None and want in ("lo", "both"):
            out = torch.empty(m, max(n, n_store), dtype=ops.TORCH_DTYPE[dt], device=self.dev)
        if out_f32 is None and want in ("f32", "both"):
            out_f32 = self.f32(m, n)
        sl = None if slope is None else self.pk.slope(slope, n) if not torch.is_tensor(slope) else slope
        kw = {}
        if conv is not None:
            stride, pad, lin, lout = conv
            kw = dict(taps=e["taps"], stride=stride, pad=pad, lin=lin, lout=lout)
        sk = ops._SPLITK[0]
        if sk is not None and h2 and m <= ops.SPLITK_MAX_ROWS and self.dev.type == "cuda":
            kw["splitk"] = sk.get(self.dev)       # few rows (ONE clip: 64): the launch may split its K range (ops.SplitKScratch)
        ops.gemm(dt, a, e["w"], e["b"], sl, res, out, out_f32, out_t, n=n, cp=e["cp"], n_store=n_store,
                 t_col0=t_col0, t_rows=t_rows, res_first=res_first, m=m, k_real=e.get("k_real"), w_scale=e.get("ws", 1.0),
                 res_h2=bool(res_h2 and h2), **kw, **({} if (ln is None and res_ln is None and stats_out is None)
                                                            else dict(ln=ln, res_ln=res_ln, stats_out=stats_out)))
        return out, out_f32

    # ---- folded LayerNorms (`fold_ln`): an `_X` whose `.ln` is set stands for LayerNorm(x.a) without that tensor existing ----
    def gemm_ln(self, x, key, **kw):
        """Contraction whose operand is the `_X` x: a folded LayerNorm's consumer runs on the raw sum with the folded operands of `key`."""
        if x.ln is None:
            return self.gemm(x.a, key, **kw)
        stats, nkey = x.ln
        e = self.pk.w[key + "@" + nkey]
        return self.gemm(x.a, key, w=e, ln=(stats, e["c"]), **kw)

    def res_of(self, x):
        """The residual keywords of a sub-layer's output contraction for the `_X` x."""
        if x.ln is None:
            return dict(res=x.r, res_h2=x.h2r)
        stats, nkey = x.ln
        n = self.pk.w[nkey]
        return dict(res=x.a, res_h2=True, res_ln=(stats, n["g"], n["b"]))

    def gemm_s(self, a, key, x, stats=False):
        """The pre-norm sum x + a W^T + b of a sub-layer.  stats (the LayerNorm behind it is folded): -> `_S` (the sum as an EMAGE_H2 image
        + its partial row statistics, written by the contraction's epilogue); else the tensor `gemm_r` returns."""
        if not stats:
            return self.gemm_r(a, key, **self.res_of(x))
        e = self.pk.w[key]
        st = torch.empty(a.shape[0], e["n"] // 32, 2, dtype=torch.float32, device=self.dev)
        out, _ = self.gemm(a, key, want="lo", stats_out=st, **self.res_of(x))
        return _S(out, st)

    # ---- the two forms of an activation: `.a` feeds contractions (storage type of the mode), `.r` carries the residual stream
    # (the same tensor, except in EMAGE_H2 mode where it is the float32 twin) ----
    def gemm_x(self, a, key, **kw):
        """Contraction whose result is both an operand and a residual: -> _X."""
        lo, f = self.gemm(a, key, want="both" if self.h2 else "lo", **kw)
        return _X(lo, f if self.h2 else lo)

    def gemm_r(self, a, key, **kw):
        """Contraction whose result is only read at residual precision (a pre-norm sum, attention q / k): -> tensor."""
        lo, f = self.gemm(a, key, want="f32" if self.h2 else "lo", **kw)
        return f if self.h2 else lo

    def conv3(self, a, key, t, **kw):
        return self.gemm(a, key, conv=(1, 1, t, t), **kw)

    def vt_buffer(self, b, rows, tk):
        tp = _rup(tk, 32)
        alloc = torch.empty if tp == tk else torch.zeros      # padded key columns must stay finite
        return alloc(b, rows, tp, dtype=self.tdt, device=self.dev)


class _X:
    """An activation in its two forms (see _Ctx.gemm_x); h2r: `.r` is an EMAGE_H2 image too (then it IS `.a`).
    ln = (partial row statistics, norm key): the activation is LayerNorm_key(.a) and has NOT been computed — `.a` is the raw pre-norm
    sum (an EMAGE_H2 image); its consumers fold the norm (`_Ctx.gemm_ln` / `res_of`)."""
    __slots__ = ("a", "r", "h2r", "ln")

    def __init__(self, a, r, h2r=False, ln=None):
        self.a, self.r, self.h2r, self.ln = a, r, h2r, ln


class _S:
    """A pre-norm sum whose LayerNorm will be folded: the EMAGE_H2 image and its (M, C / 32, 2) partial row statistics."""
    __slots__ = ("img", "stats")

    def __init__(self, img, stats):
        self.img, self.stats = img, stats


class _Memory(NamedTuple):
    """The cross-attention memory (Tk frames per clip) of a stack of `n` decoder layers, in one of two forms (`_stack_memory` decides which).
    Projected: k (B*Tk, n*d) keys and vt (B, n*d, Tp) V^T of every layer, as `_memory_kv` writes them.  Site (`_memory_site`): k / vt are
    None — each layer's launch contracts the feature image img (B*Tk, km) with the stack's composed K / V operand cx.pk.w[kv_key] itself."""
    k: object
    vt: object
    img: object
    kv_key: object
    n: int
    tk: int
    index: int = 0

    def layer(self, i):
        """What `_decoder_layer` takes for layer i of the stack."""
        return self._replace(index=i)

    def kv(self):
        """This layer's projected memory as the attention launches take it: the (B*Tk, d) view of its keys, the view of the V^T buffer at
        its first row, and that buffer's rows per clip."""
        vt_rows, i = self.vt.shape[1], self.index
        d = vt_rows // self.n
        return self.k[:, i * d:(i + 1) * d], self.vt[:, i * d:], vt_rows

    def clips(self, clip0, n):
        """The memory of clips [clip0, clip0 + n) (row views)."""
        rows = lambda x, per: None if x is None else x[clip0 * per:(clip0 + n) * per]
        return self._replace(k=rows(self.k, self.tk), vt=rows(self.vt, 1), img=rows(self.img, self.tk))


def _conv_encoder(cx: _Ctx, prefix, x_lo, t, n_layer, length, want_f32):
    """VQEncoderV5 / V6 (P:189-235) on a (M, Cp) operand; returns (lo (M,Cp(length)), f32 (M,length)|None)."""
    lp = _rup(length)
    h, hf = x_lo, None
    for i in range(n_layer):
        h, _ = cx.conv3(h, f"{prefix}.main.{3 * i}", t, slope=0.2, n_store=lp)
        r, _ = cx.conv3(h, f"{prefix}.main.{3 * i + 2}.model.0", t, slope=0.2, n_store=lp)
        last = i == n_layer - 1
        h, hf = cx.conv3(r, f"{prefix}.main.{3 * i + 2}.model.2", t, res=h, res_h2=cx.h2, n_store=lp,
                         want="both" if (last and want_f32) else "lo")
    return h, hf


def _conv_decoder(cx: _Ctx, prefix, z_lo, t, n_layer, length, out_dim):
    """VQDecoderV5 (P:237-261): (M, Cp(length)) -> fp32 (M, out_dim)."""
    lp, dp = _rup(length), _rup(out_dim)
    h = z_lo
    for i in range(2):
        r, _ = cx.conv3(h, f"{prefix}.main.{i}.model.0", t, slope=0.2, n_store=lp)
        h, _ = cx.conv3(r, f"{prefix}.main.{i}.model.2", t, res=h, res_h2=cx.h2, n_store=lp)
    for i in range(n_layer):
        h, _ = cx.conv3(h, f"{prefix}.main.{2 + 2 * i}", t, slope=0.2, n_store=dp if i == n_layer - 1 else lp)
    _, out = cx.conv3(h, f"{prefix}.main.{2 + 2 * n_layer}", t, want="f32")
    return out


def _pack_conv_encoder(pk, prefix, n_layer):
    for i in range(n_layer):
        pk.conv(f"{prefix}.main.{3 * i}", f"{prefix}.main.{3 * i}")
        pk.conv(f"{prefix}.main.{3 * i + 2}.model.0", f"{prefix}.main.{3 * i + 2}.model.0")
        pk.conv(f"{prefix}.main.{3 * i + 2}.model.2", f"{prefix}.main.{3 * i + 2}.model.2")


def _pack_conv_decoder(pk, prefix, n_layer):
    for i in range(2):
        pk.conv(f"{prefix}.main.{i}.model.0", f"{prefix}.main.{i}.model.0")
        pk.conv(f"{prefix}.main.{i}.model.2", f"{prefix}.main.{i}.model.2")
    for i in range(n_layer + 1):
        pk.conv(f"{prefix}.main.{2 + 2 * i}", f"{prefix}.main.{2 + 2 * i}")


# ======================================================================================
# EmageVAEConv / EmageVQVAEConv  (M:19-70)
# ======================================================================================
class _Tokenizer(_EmageModule):
    """The motion tokenizers are frozen unless asked otherwise: the EMAGE trainer relies on it (T:233-245), so `.train()` on a fresh
    instance raises.  `unfreeze()` makes THIS instance trainable — `.train()` then switches `forward` to the differentiable train-mode
    forward (pantomatrix_amd/training_vq.py); `freeze()` puts it back into eval mode and restores the raise.  The eval-mode entry points
    (`forward`, `map2index`, `map2latent`, `decode`, `decode_from_latent`) are the same code in both states."""

    def train(self, mode=True):
        if mode and not self._trainable:
            raise NotImplementedError(f"{type(self).__name__} is frozen (the reference keeps its VQ-VAEs frozen while EMAGE trains, "
                                      "train_emage_audio.py:233-245): call .unfreeze() first to train this tokenizer")
        return super().train(mode)

    def unfreeze(self):
        self.__dict__["_trainable"] = True
        return self

    def freeze(self):
        self.eval()
        self.__dict__.pop("_trainable", None)
        self.__dict__.pop("_train_fwd", None)
        return self


class EmageVAEConv(_Tokenizer):
    config_class = EmageVAEConvConfig
    base_model_prefix = "emage_vaeconv"
    _spec_fn = staticmethod(spec.vae_spec)

    def _pack(self, pk):
        _pack_conv_encoder(pk, "encoder", self.config.vae_layer)
        _pack_conv_decoder(pk, "decoder", self.config.vae_layer)

    def forward(self, inputs):
        if self.training:
            from . import training_vq
            return training_vq.train_forward(self, inputs)
        c = self.config
        cx = _Ctx(self._engine())
        b, t, d = inputs.shape
        x = ops.cast_pad(cx.dt, inputs.reshape(b * t, d).float().contiguous(), _rup(d))
        h, _ = _conv_encoder(cx, "encoder", x, t, c.vae_layer, c.vae_length, False)
        rec = _conv_decoder(cx, "decoder", h, t, c.vae_layer, c.vae_length, c.vae_test_dim)
        return {"rec_pose": rec.view(b, t, c.vae_test_dim)}



class EmageVQVAEConv(_Tokenizer):
    config_class = EmageVQVAEConvConfig
    base_model_prefix = "emage_vqvaeconv"
    _spec_fn = staticmethod(spec.vqvae_spec)

    def _pack(self, pk):
        _pack_conv_encoder(pk, "encoder", self.config.vae_layer)
        _pack_conv_decoder(pk, "decoder", self.config.vae_layer)
        pk.w["codebook"] = pk.f32("quantizer.embedding.weight")

    # -- pieces --------------------------------------------------------------------------
    def _encode(self, cx, inputs):
        c = self.config
        b, t, d = inputs.shape
        x = ops.cast_pad(cx.dt, inputs.reshape(b * t, d).float().contiguous(), _rup(d))
        _, pre = _conv_encoder(cx, "encoder", x, t, c.vae_layer, c.vae_length, True)
        return pre                                                  # fp32 (B*T, vae_length)

    def _nearest(self, cx, z2d, out=None):
        assert z2d.shape[-1] == self.config.vae_length               # P:145,159
        return ops.vq_argmin(z2d, cx.pk.w["codebook"], out=out)

    def _decode_idx(self, cx, idx, b, t):
        """idx: (B*T,) list or a (B, T) view of a longer code buffer (read in place, ops.index_view)."""
        c = self.config
        zq = ops.gather_rows(cx.pk.w["codebook"], idx, cx.dt, _rup(c.vae_length))
        return _conv_decoder(cx, "decoder", zq, t, c.vae_layer, c.vae_length, c.vae_test_dim)   # fp32 (B*T, dim)

    # -- reference API ---------------------------------------------------------------------
    def map2index(self, inputs):                                     # M:47-50
        cx = _Ctx(self._engine())
        return self._nearest(cx, self._encode(cx, inputs)).view(inputs.shape[0], -1)

    def map2latent(self, inputs):                                    # M:51-55
        cx = _Ctx(self._engine())
        idx = self._nearest(cx, self._encode(cx, inputs))
        return ops.gather_rows(cx.pk.w["codebook"], idx, F32).view(inputs.shape[0], inputs.shape[1], -1)

    def decode(self, index):                                         # M:56-59
        cx = _Ctx(self._engine())
        b, t = index.shape
        return self._decode_idx(cx, index, b, t).view(b, t, -1)

    def decode_from_latent(self, latent):                            # M:60-70
        cx = _Ctx(self._engine())
        b, t, d = latent.shape
        idx = self._nearest(cx, latent.reshape(b * t, d).float().contiguous())
        return self._decode_idx(cx, idx, b, t).view(b, t, -1)

    def forward(self, inputs):                                       # M:42-46 (values in eval mode; differentiable after unfreeze().train())
        if self.training:
            from . import training_vq
            return training_vq.train_forward(self, inputs)
        cx = _Ctx(self._engine())
        b, t, _ = inputs.shape
        pre = self._encode(cx, inputs)
        idx = self._nearest(cx, pre)
        zq = ops.gather_rows(cx.pk.w["codebook"], idx, F32)
        # Quantizer.forward's scalars (P:151,154-155) are training diagnostics: tiny reductions, done with torch
        diff = torch.mean((zq - pre) ** 2)
        loss = diff + self.config.vae_quantizer_lambda * diff
        e_mean = torch.bincount(idx, minlength=self.config.vae_codebook_size).float() / idx.numel()
        perplexity = torch.exp(-torch.sum(e_mean * torch.log(e_mean + 1e-10)))
        rec = self._decode_idx(cx, idx, b, t)
        return {"poses_feat": zq.view(b, t, -1), "embedding_loss": loss, "perplexity": perplexity,
                "rec_pose": rec.view(b, t, -1)}



# ======================================================================================
# EmageVQModel  (M:72-205)
# ======================================================================================
# joint partition of the 55 SMPL-X joints, M:75-90 (boolean masks in the reference); the hands are joints 25-54 (M:103)
JOINT_MASK_UPPER = tuple(j in (3, 6, 9, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21) for j in range(55))
JOINT_MASK_LOWER = tuple(j in (0, 1, 2, 4, 5, 7, 8, 10, 11) for j in range(55))
JOINT_MASK_HANDS = tuple(25 <= j < 55 for j in range(55))


class EmageVQModel(torch.nn.Module):
    def __init__(self, face_model, upper_model, hands_model, lower_model, global_model):
        super().__init__()
        self.joint_mask_upper = list(JOINT_MASK_UPPER)
        self.joint_mask_lower = list(JOINT_MASK_LOWER)
        self.vq_model_face = face_model
        self.vq_model_upper = upper_model
        self.vq_model_hands = hands_model
        self.vq_model_lower = lower_model
        self.global_motion = global_model
        self._templates = {}                       # device index tensors of the joint partition, per device

    def _models(self):
        return (self.vq_model_face, self.vq_model_upper, self.vq_model_hands, self.vq_model_lower, self.global_motion)

    def set_precision(self, precision):
        for m in self._models():
            m.set_precision(precision)
        return self

    def set_activation_shift(self, shift):
        for m in self._models():
            m.set_activation_shift(shift)
        return self

    @property
    def activation_shift(self):
        return max(m.activation_shift for m in self._models())

    @property
    def precision(self):
        return self.vq_model_face.precision

    def spilt_inputs(self, smplx_body_rot6d, expression, tar_contact=None, tar_trans=None):     # (sic) M:97-108
        bs, t, j6 = smplx_body_rot6d.shape
        r = smplx_body_rot6d.reshape(bs, t, j6 // 6, 6)
        dev = smplx_body_rot6d.device
        key = ("joint_index", str(dev))
        if key not in self._templates:               # device index tensors, built once (never inside a graph capture)
            self._templates[key] = tuple(torch.tensor([j for j in range(55) if mk[j]], dtype=torch.long, device=dev)
                                         for mk in (self.joint_mask_upper, self.joint_mask_lower))
        up, lo = self._templates[key]
        face = torch.cat([r[:, :, 22], expression], dim=2)
        upper = r.index_select(2, up).reshape(bs, t, 78)
        hands = r[:, :, 25:55].reshape(bs, t, 180)
        lower = r.index_select(2, lo).reshape(bs, t, 54)
        tar_contact = torch.zeros(bs, t, 4, device=dev) if tar_contact is None else tar_contact
        tar_trans = torch.zeros(bs, t, 3, device=dev) if tar_trans is None else tar_trans
        return dict(face=face, upper=upper, hands=hands, lower=torch.cat([lower, tar_trans, tar_contact], dim=2))

    def map2index(self, smplx_body_rot6d, expression, tar_contact=None, tar_trans=None):        # M:110-116
        x = self.spilt_inputs(smplx_body_rot6d, expression, tar_contact, tar_trans)
        return {p: getattr(self, f"vq_model_{p}").map2index(x[p]) for p in ("face", "upper", "hands", "lower")}

    def map2latent(self, smplx_body_rot6d, expression, tar_contact=None, tar_trans=None):       # M:118-124
        x = self.spilt_inputs(smplx_body_rot6d, expression, tar_contact, tar_trans)
        return {p: getattr(self, f"vq_model_{p}").map2latent(x[p]) for p in ("face", "upper", "hands", "lower")}

    def decode(self, face_index=None, upper_index=None, hands_index=None, lower_index=None,
               face_latent=None, upper_latent=None, hands_latent=None, lower_latent=None,
               get_global_motion=False, ref_trans=None):                                         # M:126-193
        bs = t = None
        for x in (face_index, upper_index, hands_index, lower_index, face_latent, upper_latent, hands_latent, lower_latent):
            if x is not None:
                bs, t = x.shape[:2]
                break
        m = bs * t
        dev = self.vq_model_face.device
        todo = (("lower", lower_index, lower_latent), ("hands", hands_index, hands_latent),
                ("upper", upper_index, upper_latent), ("face", face_index, face_latent))
        trans = [None]

        def scan(lower_mix):
            trans[0] = self.get_global_motion(lower_mix.view(bs, t, -1), ref_trans)

        parts = self._part_chains(todo, bs, t, scan if get_global_motion else None)
        aa, motion, expr = ops.merge_parts(parts["face"], parts["upper"], parts["hands"], parts["lower"], m, dev)
        return dict(expression=expr.view(bs, t, 100), all_motion4inference=motion.view(bs, t, 337),
                    motion_axis_angle=aa.view(bs, t, 165), trans=trans[0])

    def _decode_segments(self, face_index=None, upper_index=None, hands_index=None, lower_index=None):
        """A batch of code SEGMENTS (B, T) -> (axis-angle (B * T, 165), expressions (B * T, 100), the global model's output (B * T, 61) whose
        columns 54 .. 56 are x velocity, height, z velocity): `decode(get_global_motion=True)` without the scan over the velocities, which a
        stream continues across segments (pantomatrix_amd/streaming.py).  The same part chains as `decode`."""
        bs, t = next(x for x in (face_index, upper_index, hands_index, lower_index) if x is not None).shape[:2]
        todo = (("lower", lower_index, None), ("hands", hands_index, None), ("upper", upper_index, None), ("face", face_index, None))
        vel = [None]

        def velocities(lower_mix):
            vel[0] = self.global_motion.forward(lower_mix.view(bs, t, -1))["rec_pose"].view(bs * t, -1)

        parts = self._part_chains(todo, bs, t, velocities)
        aa, _motion, expr = ops.merge_parts(parts["face"], parts["upper"], parts["hands"], parts["lower"], bs * t, self.vq_model_face.device,
                                            want_motion=False)
        return aa, expr, vel[0]

    def _part_chains(self, todo, bs, t, after_lower):
        """The four part decoders of `decode` on (B, T) codes / latents -> {part: fp32 (B * T, dim) or None}; after_lower: what follows the
        lower stream inside its chain (the global-translation model), called with the lower part's output, or None."""
        m = bs * t
        parts = {}
        dev = self.vq_model_face.device
        # every part's operand set is packed BEFORE the chains below are entered: a packing is torch arithmetic + launches
        # of its own and must not run at record time inside a lock-step chain, where only emage ops are deferred
        engines = {name: getattr(self, f"vq_model_{name}")._engine() for name, index, latent in todo if index is not None or latent is not None}
        if after_lower is not None:
            self.global_motion._engine()

        def part_chain(name, index, latent):
            model = getattr(self, f"vq_model_{name}")
            if index is not None:
                cx = _Ctx(engines[name])
                parts[name] = model._decode_idx(cx, index, bs, t)
            elif latent is not None:
                cx = _Ctx(engines[name])
                idx = model._nearest(cx, latent.reshape(m, -1).float().contiguous())
                parts[name] = model._decode_idx(cx, idx, bs, t)
            else:
                parts[name] = None
            if name == "lower" and after_lower is not None:
                lower_mix = parts["lower"]
                if lower_mix is None:   # zeros pose: identity rot6d + zero trans/contact (M:174-177)
                    lower_mix = torch.tensor([1.0, 0, 0, 0, 1, 0] * 9 + [0.0] * 7, device=dev).repeat(m, 1)
                after_lower(lower_mix)

        # the four part decoders are independent chains of the same shapes on different weights (the global-translation AE follows the
        # lower stream): walked in lock step, their contractions share launches (4 x 8 launches with one block per CU -> 8 with four);
        # group_gemms = False: one stream lane per chain, one launch per contraction
        if getattr(self.vq_model_face, "group_gemms", True) and dev.type == "cuda":
            with ops.lockstep() as ls:
                for name, index, latent in todo:
                    with ls.chain():
                        part_chain(name, index, latent)
        else:
            with Fork(dev, 4, getattr(self.vq_model_face, "concurrent", True)) as fk:
                for lane, (name, index, latent) in enumerate(todo):
                    with fk.lane(lane):
                        part_chain(name, index, latent)
        return parts

    def get_global_motion(self, lower_body, ref_trans):                                          # M:195-205
        bs, t, _ = lower_body.shape
        rec = self.global_motion.forward(lower_body)["rec_pose"]                                 # (B,T,61) fp32
        # M:198-200: a 2-D ref_trans is shared by every clip; only its first frame is used.  Views, no copies:
        init = ref_trans[0:1] if ref_trans.dim() == 2 else ref_trans[:, 0, :]
        init = init.to(device=rec.device, dtype=torch.float32)
        return ops.velocity_to_position(rec.view(bs * t, -1), 54, init, 1 / 30, bs, t)


# ======================================================================================
# WavEncoder (P:263-314; the DisCo / CaMN model files carry the same module with other widths)
# ======================================================================================
class _WavEncoderMixin:
    """Six BasicBlocks of Conv1d(k=15) + BatchNorm + LeakyReLU(0.01) with conv+BN shortcuts, on the raw waveform.
    `_wav_blocks()` gives the geometry [(cin, cout, stride, pad, has_shortcut)]; eval BatchNorm is folded into the convs,
    block 0 (Cin = 1) of every encoder of the model is one `emage_wav_conv_in` launch, each later block is two
    implicit-GEMM launches (conv1 stacked with its shortcut conv; conv2 with the shortcut add + activation fused)."""

    def _wav_blocks(self):
        raise NotImplementedError

    def _wav_clip_chunk(self, cx, n_seq, lens, width=None):
        """Sequences per launch so that the largest intermediate (block 0's (seq * L0, n_enc*2q) output) stays below the
        2 GiB a kernel operand may span (32-bit buffer offsets, include/emage_hip.h: emage_gemm)."""
        es = 2 if cx.tdt == torch.bfloat16 else 4
        per_seq = lens[0] * (width or cx.pk.w["wav_in"]["w"].shape[0]) * es
        return max(1, min(n_seq, ((1 << 31) - (1 << 20)) // per_seq))

    def _pack_wav_encoders(self, pk, encoders):
        w0, b0, s0 = [], [], []
        for enc in encoders:
            for i, (cin, cout, stride, pad, ds) in enumerate(self._wav_blocks()):
                base = f"{enc}.feat_extractor.{i}"
                if i == 0:
                    for conv, bn, sl in ((base + ".conv1", base + ".bn1", 0.01), (base + ".downsample.0", base + ".downsample.1", 1.0)):
                        w, b = pk.folded(conv, bn)
                        w0.append(w.reshape(cout, _WAV_TAPS))
                        b0.append(b)
                        s0.append(torch.full((cout,), sl, device=pk.device))
                else:
                    pk.conv(base + ".conv1", base + ".conv1", fold_bn=base + ".bn1",
                            extra=(base + ".downsample.0", base + ".downsample.1") if ds else None, dt=pk.wav_dt)
                    n1 = cout * (2 if ds else 1)
                    pk.w[base + ".conv1"]["slope"] = torch.cat([torch.full((cout,), 0.01, device=pk.device),
                                                                torch.ones(n1 - cout, device=pk.device)]).contiguous()
                pk.conv(base + ".conv2", base + ".conv2", fold_bn=base + ".bn2", dt=pk.wav_dt)
                dev = pk.device
                lrelu, ident = (lambda n: torch.full((n,), 0.01, device=dev)), (lambda n: torch.ones(n, device=dev))
                if cout == _NARROW:                              # conv2 (stride 1, Cout -> Cout) over position pairs
                    w, b = pk.folded(base + ".conv2", base + ".bn2")
                    pk.conv_pairs(base + ".conv2.pairs", w, b, lrelu(cout), 1, _WAV_TAPS // 2)
                if i > 0 and cin == _NARROW:                     # conv1 (+ shortcut conv) reading narrow rows
                    w1, b1 = pk.folded(base + ".conv1", base + ".bn1")
                    if not ds:
                        pk.conv_pairs(base + ".conv1.pairs", w1, b1, lrelu(cout), stride, pad)
                    else:
                        wd, bd = pk.folded(base + ".downsample.0", base + ".downsample.1")
                        if cout == _NARROW:                      # two launches: both results must be contiguous narrow tensors
                            pk.conv_pairs(base + ".conv1.pairs", w1, b1, lrelu(cout), stride, pad)
                            pk.conv_pairs(base + ".downsample.pairs", wd, bd, ident(cout), stride, pad)
                        else:
                            pk.conv_pairs(base + ".conv1.pairs", torch.cat([w1, wd], 0), torch.cat([b1, bd]),
                                          torch.cat([lrelu(cout), ident(cout)]), stride, pad)
        pk.w["wav_in"] = dict(w=torch.cat(w0, 0).float().contiguous(), b=torch.cat(b0).float().contiguous(),
                              slope=torch.cat(s0).float().contiguous())

    def _wav_lengths(self, l):
        """Frame counts after each of the 6 BasicBlocks (P:301-306) for an l-sample window."""
        lens, cur = [], l
        for (_ci, _co, stride, pad, _ds) in self._wav_blocks():
            cur = (cur + 2 * pad - _WAV_TAPS) // stride + 1
            lens.append(cur)
        if min(lens) <= 0:
            raise RuntimeError(f"audio window of {l} samples is too short for the WavEncoder")
        return lens

    def _wav_first_layer(self, cx, audio, lens, nwin=1, hop=0, win_len=None):
        """Block 0's conv1 and downsample shortcut of EVERY encoder of the model in one launch: (nwin*B*L0, n_enc*2q) =
        [enc0 conv1 | enc0 shortcut | enc1 conv1 | enc1 shortcut]; `nwin` sliding windows per clip are read in place."""
        blocks = self._wav_blocks()
        w_in = cx.pk.w["wav_in"]
        y0 = cx.lo(nwin * audio.shape[0] * lens[0], w_in["w"].shape[0])
        ops.wav_conv_in(cx.wdt, audio, w_in["w"], w_in["b"], w_in["slope"], y0, lens[0], blocks[0][2], blocks[0][3],
                        nwin=nwin, hop=hop, win_len=win_len)
        return y0

    def _wav_block0_fused(self):
        """Block 0 runs as ONE launch per encoder (`emage_wav_block0`) when its width is one the slab kernel is built for."""
        # measured per kernel (profiles/r02_bench_slab.txt): the fused block 0 wins in f16x3 only (786 vs 915 us); in bf16 / fp32
        # its VALU first layer costs more than the tensor round trip it saves
        blocks = self._wav_blocks()
        return self.slab_convs and self._dt == F16X3 and ops.conv_slab_supported(blocks[0][1], _WAV_TAPS, 1)

    def _wav_encoder_chain(self, cx, enc, e, y0, b, lens, dest=None, wav=None, nwin=1, hop=0, win_len=None):
        """Blocks 0..5 of one WavEncoder (P:283-314).  Block 0 is either the fused launch on the raw waveform (`wav`
        given) or starts from the shared first-layer tensor `y0`; stride-1 convolutions of 64 / 128 channels run with
        their input slab resident in LDS (`emage_conv_slab`), the others as implicit GEMMs.  Returns (B*T', C_out);
        written straight into `dest` (a 2-D view) when its row count matches.  `b` counts sequences (windows x clips)."""
        blocks = self._wav_blocks()
        k, q = _WAV_TAPS, blocks[0][1]
        w_in = cx.pk.w["wav_in"]
        x, lin = None, None
        for i, (cin, cout, stride, pad, ds) in enumerate(blocks):
            base = f"{enc}.feat_extractor.{i}"
            lout = lens[i]
            c2 = cx.pk.w[base + ".conv2"]
            slab2 = self.slab_convs and ops.conv_slab_supported(cout, k, 1)
            if i == 0 and wav is not None:
                rows = slice(e * 2 * q, e * 2 * q + q), slice(e * 2 * q + q, (e + 1) * 2 * q)
                x = cx.lo(b * lout, cout)
                ops.wav_block0(cx.wgdt, wav, w_in["w"][rows[0]], w_in["b"][rows[0]], 0.01, w_in["w"][rows[1]], w_in["b"][rows[1]],
                               stride, pad, c2["w"], c2["b"], cx.pk.slope(0.01, cout), k, k // 2, x, lout,
                               nwin=nwin, hop=hop, win_len=win_len, w_scale=c2.get("ws", 1.0))
                lin = lout
                continue
            if i == 0:
                y1, sc = y0[:, e * 2 * q: e * 2 * q + q], y0[:, e * 2 * q + q: (e + 1) * 2 * q]
            else:
                ent = cx.pk.w[base + ".conv1"]
                if self.slab_convs and not ds and ops.conv_slab_supported(cout, k, stride) and cin == cout:
                    y = cx.lo(b * lout, cout)
                    ops.conv_slab(cx.wgdt, x, ent["w"], ent["b"], ent["slope"], None, y, nseq=b, l=lout, taps=k, pad=pad, w_scale=ent.get("ws", 1.0))
                else:
                    y, _ = cx.gemm(x, base + ".conv1", slope=ent["slope"], conv=(stride, pad, lin, lout), m=b * lout, n_store=_rup(ent["n"]))
                y1, sc = (y[:, :cout], y[:, cout:2 * cout]) if ds else (y[:, :cout], x)
            last = i == len(blocks) - 1
            out = dest if (last and dest is not None and dest.shape[0] == b * lout) else None
            if slab2:
                x = out if out is not None else cx.lo(b * lout, cout)
                ops.conv_slab(cx.wgdt, y1, c2["w"], c2["b"], cx.pk.slope(0.01, cout), sc, x, nseq=b, l=lout, taps=k, pad=k // 2, w_scale=c2.get("ws", 1.0))
            else:
                x, _ = cx.gemm(y1, base + ".conv2", slope=0.01, res=sc, res_first=True, conv=(1, k // 2, lout, lout),
                               m=b * lout, out=out, n_store=0 if out is not None else _rup(cout))
                x = x[:, :cout] if x.shape[1] != cout else x
            lin = lout
        return x

    # ---- narrow (32-channel) blocks as convolutions over position pairs (DisCo / CaMN) ------------------------------------
    def _wav_pairs_ok(self, lens):
        """The pair form needs the slab kernel, a narrow first block, and an even frame count wherever rows are paired."""
        blocks = self._wav_blocks()
        if not (self.slab_convs and blocks[0][1] == _NARROW and ops.conv_slab_supported(2 * _NARROW, _WAV_TAPS, 1)):
            return False
        for i, (cin, cout, stride, pad, ds) in enumerate(blocks):
            if cout == _NARROW and lens[i] % 2:
                return False
            if i > 0 and cin == _NARROW and stride > 1 and (stride % 2 or pad):
                return False
        return True

    def _wav_first_layer_pairs(self, cx, audio, lens):
        """Block 0's conv1 and shortcut of the (single) narrow encoder as two contiguous (B*L0, 32) tensors."""
        blocks = self._wav_blocks()
        q, w_in = blocks[0][1], cx.pk.w["wav_in"]
        outs = []
        for r in (slice(0, q), slice(q, 2 * q)):
            y = cx.lo(audio.shape[0] * lens[0], q)
            ops.wav_conv_in(cx.wdt, audio, w_in["w"][r], w_in["b"][r], w_in["slope"][r], y, lens[0], blocks[0][2], blocks[0][3])
            outs.append(y)
        return outs

    def _wav_encoder_chain_pairs(self, cx, enc, y1, sc, b, lens, dest=None):
        """`_wav_encoder_chain` for an encoder whose first blocks are 32 channels wide: those blocks' rows are read and
        written as (L/2, 64) pair rows by the 64-channel kernels (`_Packed.conv_pairs`) instead of zero-padded to 64
        channels — a quarter of the padded path's MFMA work and half its activation bytes."""
        blocks = self._wav_blocks()
        k = _WAV_TAPS
        pairs = lambda t: t.view(-1, 2 * _NARROW)

        def slab_pairs(a, key, res, l):
            e = cx.pk.w[key]
            out = cx.lo(a.shape[0], _NARROW)
            ops.conv_slab(cx.wgdt, pairs(a), e["w"], e["b"], e["slope"], None if res is None else pairs(res), pairs(out),
                          nseq=b, l=l // 2, taps=e["taps"], pad=e["pad"], w_scale=e.get("ws", 1.0))
            return out

        x, lin = None, None
        for i, (cin, cout, stride, pad, ds) in enumerate(blocks):
            base = f"{enc}.feat_extractor.{i}"
            lout = lens[i]
            if i > 0:
                if cin != _NARROW:                                   # wide input: the regular forms
                    ent = cx.pk.w[base + ".conv1"]
                    if not ds and ops.conv_slab_supported(cout, k, stride) and cin == cout:
                        y = cx.lo(b * lout, cout)
                        ops.conv_slab(cx.wgdt, x, ent["w"], ent["b"], ent["slope"], None, y, nseq=b, l=lout, taps=k, pad=pad, w_scale=ent.get("ws", 1.0))
                    else:
                        y, _ = cx.gemm(x, base + ".conv1", slope=ent["slope"], conv=(stride, pad, lin, lout), m=b * lout, n_store=_rup(ent["n"]))
                    y1, sc = (y[:, :cout], y[:, cout:2 * cout]) if ds else (y[:, :cout], x)
                elif not ds:                                         # 32 -> 32, stride 1
                    y1, sc = slab_pairs(x, base + ".conv1.pairs", None, lout), x
                else:                                                # strided, reading pair rows
                    e1 = cx.pk.w[base + ".conv1.pairs"]
                    cv = (e1["stride"], 0, lin // 2, lout)
                    if cout == _NARROW:
                        y1, _ = cx.gemm(pairs(x), None, w=e1, slope=e1["slope"], conv=cv, m=b * lout)
                        ed = cx.pk.w[base + ".downsample.pairs"]
                        sc, _ = cx.gemm(pairs(x), None, w=ed, slope=ed["slope"], conv=cv, m=b * lout)
                    else:
                        y, _ = cx.gemm(pairs(x), None, w=e1, slope=e1["slope"], conv=cv, m=b * lout)
                        y1, sc = y[:, :cout], y[:, cout:2 * cout]
            last = i == len(blocks) - 1
            out = dest if (last and dest is not None and dest.shape[0] == b * lout) else None
            if cout == _NARROW:
                x = slab_pairs(y1, base + ".conv2.pairs", sc, lout)
            else:
                c2 = cx.pk.w[base + ".conv2"]
                if ops.conv_slab_supported(cout, k, 1):
                    x = out if out is not None else cx.lo(b * lout, cout)
                    ops.conv_slab(cx.wgdt, y1, c2["w"], c2["b"], cx.pk.slope(0.01, cout), sc, x, nseq=b, l=lout, taps=k, pad=k // 2, w_scale=c2.get("ws", 1.0))
                else:
                    x, _ = cx.gemm(y1, base + ".conv2", slope=0.01, res=sc, res_first=True, conv=(1, k // 2, lout, lout),
                                   m=b * lout, out=out, n_store=0 if out is not None else _rup(cout))
                    x = x[:, :cout] if x.shape[1] != cout else x
            lin = lout
        return x


# ======================================================================================
# EmageAudioModel  (M:207-490)
# ======================================================================================
# the stacks' memory K / V operands composed with the memory projection in front of them (`compose_memory`): key "<kv entry>@<projection>"
_BODY_KV, _FACE_KV = "cross.kv_all@audio_body_motion_proj", "face.kv_all@audio_face_motion_proj"
# the two decoder stacks' memory: (composed K / V operand, the memory projection it absorbs, the plain K / V operand, layers)
_STACKS = {"body": (_BODY_KV, "audio_body_motion_proj", "cross.kv_all", spec.N_CROSS_LAYERS),
           "face": (_FACE_KV, "audio_face_motion_proj", "face.kv_all", spec.N_FACE_LAYERS)}


class EmageAudioModel(_WavEncoderMixin, _EmageModule):
    config_class = EmageAudioConfig
    base_model_prefix = "emage_audio"
    _spec_fn = staticmethod(spec.audio_model_spec)
    _trainable = True        # model.train(); out = model(...); loss.backward() — pantomatrix_amd/training.py: train_forward

    def _wav_blocks(self):
        return spec.wav_encoder_blocks(self.config.audio_f)

    # ---- weight packing ----------------------------------------------------------------
    def _pack(self, pk):
        c = self.config
        _pack_conv_encoder(pk, "motion_encoder", spec.MOTION_ENC_LAYERS)
        pk.linear("bodyhints.fc1", ["bodyhints_face.fc1", "bodyhints_body.fc1"])
        pk.linear("bodyhints_face.fc2", ["bodyhints_face.fc2"])
        pk.linear("bodyhints_body.fc2", ["bodyhints_body.fc2"])
        for nm in ("audio_body_motion_proj", "moton_proj", "audio_face_motion_proj", "face_out_proj"):
            pk.linear(nm, [nm])
        parts = ("upper", "hands", "lower")
        pk.linear("motion2latent.fc1", [f"motion2latent_{p}.fc1" for p in parts])
        for p in parts:
            pk.linear(f"motion2latent_{p}.fc2", [f"motion2latent_{p}.fc2"])
            pk.linear(f"motion_out_proj_{p}", [f"motion_out_proj_{p}"])
            pk.linear(f"motion_cls_{p}.fc1", [f"motion_cls_{p}.fc1"])
            pk.linear(f"motion_cls_{p}.fc2", [f"motion_cls_{p}.fc2"])
        pk.linear("face_cls.fc1", ["face_cls.fc1"])
        pk.linear("face_cls.fc2", ["face_cls.fc2"])
        # transformer layers
        self._pack_layer(pk, "motion_self_encoder.layers.0", cross=False)
        cross = [f"audio_motion_cross_attn.layers.{i}" for i in range(spec.N_CROSS_LAYERS)]
        face = [f"face_motion_decoder.layers.{i}" for i in range(spec.N_FACE_LAYERS)]
        for nm in cross + face + [f"body_motion_decoder_{p}.layers.0" for p in parts]:
            self._pack_layer(pk, nm, cross=True)
        pk.in_proj("cross.kv_all", [n + ".multihead_attn" for n in cross], "kv")
        pk.in_proj("face.kv_all", [n + ".multihead_attn" for n in face], "kv")
        # LayerNorm folds (behind every plain entry, so that the packing order of those — the scale cache's key — does not depend on them)
        self._pack_folds(pk, "motion_self_encoder.layers.0", cross=False)
        for stack in (cross, face):
            for i, nm in enumerate(stack):
                self._pack_folds(pk, nm, cross=True, prev=stack[i - 1] if i else None)
        for p in parts:
            self._pack_folds(pk, f"body_motion_decoder_{p}.layers.0", cross=True)
        if not pk.train_only:        # eval-mode WavEncoders (BatchNorms folded into the convolutions); training packs the raw ones (`_train_pack`)
            self._pack_wav_encoders(pk, ("audio_encoder_face", "audio_encoder_body"))
        if pk.compose:               # behind every other operand, as the folds: the packing order of the plain entries (the scale cache's key) does not move
            pk.in_proj(_BODY_KV, [n + ".multihead_attn" for n in cross], "kv", compose="audio_body_motion_proj")
            pk.in_proj(_FACE_KV, [n + ".multihead_attn" for n in face], "kv", compose="audio_face_motion_proj")
        pk.w["pe"] = pk.f32("position_embeddings.pe")[0].contiguous()                 # (2*pose_length, d)
        pk.w["spk_body"] = pk.f32("speaker_embedding_body.weight")
        pk.w["spk_face"] = pk.f32("speaker_embedding_face.weight")
        pk.w["mask_emb"] = pk.f32("mask_embedding").reshape(-1).contiguous()

    @staticmethod
    def _pack_folds(pk, name, cross, prev=None):
        """The folded twins of a layer's LayerNorm consumers (eval-mode EMAGE_H2 only; `fold_layernorm`): key "<consumer>@<norm>".
        prev: the layer in front of it in the same stack — its last norm folds into this layer's Q / K / V projection."""
        if pk.dt != H2 or pk.train_only or pk.p[name + ".norm1.weight"].shape[0] != _FOLD_WIDTH:
            return
        last = ".norm3" if cross else ".norm2"
        if prev is not None:
            pk.in_proj(name + ".sa.qkv@" + prev + last, [name + ".self_attn"], "qkv", fold=prev + last)
        if cross:
            pk.in_proj(name + ".ca.q@" + name + ".norm1", [name + ".multihead_attn"], "q", fold=name + ".norm1")
            pk.linear(name + ".ff1@" + name + ".norm2", [name + ".linear1"], fold=name + ".norm2")
        else:
            pk.linear(name + ".ff1@" + name + ".norm1", [name + ".linear1"], fold=name + ".norm1")

    @staticmethod
    def _pack_layer(pk, name, cross):
        pk.in_proj(name + ".sa.qkv", [name + ".self_attn"], "qkv")
        pk.linear(name + ".sa.out", [name + ".self_attn.out_proj"])
        pk.norm(name + ".norm1", name + ".norm1")
        pk.norm(name + ".norm2", name + ".norm2")
        if cross:
            pk.in_proj(name + ".ca.q", [name + ".multihead_attn"], "q")
            pk.in_proj(name + ".ca.kv", [name + ".multihead_attn"], "kv")
            pk.linear(name + ".ca.out", [name + ".multihead_attn.out_proj"])
            pk.norm(name + ".norm3", name + ".norm3")
        pk.linear(name + ".ff1", [name + ".linear1"])
        pk.linear(name + ".ff2", [name + ".linear2"])

    # ---- building blocks -----------------------------------------------------------------
    # The residual stream x is stored in the compute dtype (fp32 in parity mode, bf16 in bf16 mode): each
    # sub-layer's GEMM epilogue adds the residual and writes the pre-norm sum once, LayerNorm reads it once.
    def _self_attn(self, cx, name, x, b, t, stats=False):
        """x: _X.  Returns the pre-norm sum x + out_proj(attention) at residual precision (stats: as an `_S`, for a folded LayerNorm)."""
        d, h = self.config.hidden_size, spec.N_HEAD
        m = b * t
        if self._fused_self_attn(cx, b, t, d, h):
            att = cx.lo(m, d)
            e, kw = self._site_operand(cx, name + ".sa.qkv", x, 3 * d)
            ops.qkv_attention(cx.h2dt, x.a, e["w"], e["b"], att, b, **kw)
            return cx.gemm_s(att, name + ".sa.out", x, stats)
        qk = cx.f32(m, 2 * d) if cx.h2 else cx.lo(m, 2 * d)          # the attention kernel reads float32 q / k / v^T in the split modes
        vt = cx.vt_buffer(b, d, t)
        if cx.h2:
            cx.gemm_ln(x, name + ".sa.qkv", out_f32=qk, out_t=vt, t_col0=2 * d, t_rows=t, want=None)
        else:
            cx.gemm(x.a, name + ".sa.qkv", out=qk, out_t=vt, t_col0=2 * d, t_rows=t)
        att = cx.lo(m, d)
        ops.attention(cx.gdt, qk[:, :d], qk[:, d:], vt, d, att, b, h, t, t, d // h)
        return cx.gemm_s(att, name + ".sa.out", x, stats)

    def _site_operand(self, cx, key, x, n):
        """A fused site's projection operand for the activation x — the plain one, or the one with x's pending LayerNorm folded in — and the
        scale / fold keywords its launch takes."""
        e = cx.pk.w[key] if x.ln is None else cx.pk.w[key + "@" + x.ln[1]]
        assert e["cp"] == self.config.hidden_size and e["n"] == n
        return e, dict(w_scale=e.get("ws", 1.0), ln=None if x.ln is None else (x.ln[0], e["c"]))

    def _fused_self_attn(self, cx, b, t, d, h):
        """Whether a self-attention site runs as one `ops.qkv_attention` launch: EMAGE_H2 eval forward on the GPU, a full 64-frame window, and at
        least one (clip, head) workgroup per CU — with fewer, the two-launch form spreads the projection over more CUs (B = 1: 4 workgroups) —
        and at least 16 clips (1024 rows: below, the folded projection takes a tile whose LayerNorm statistics merge in another order)."""
        if not (self.fuse_self_attention and cx.h2 and not self.training and cx.dev.type == "cuda" and ops.qkv_attention_supported(cx.h2dt, t, d, h)):
            return False
        return b >= 16 and b * h >= torch.cuda.get_device_properties(cx.dev).multi_processor_count

    def _fused_cross_attn(self, cx, b, t, tk, d, h):
        """Whether a cross-attention site runs as one `ops.q_attention` launch: EMAGE_H2 eval forward on the GPU, a full 64-frame window on a
        64-frame memory, and at least one (clip, head) workgroup per CU.  The q projection takes the 64 x 64 tile (32-row wave tiles, which the
        fused kernel's K-loop has too) at every row count up to 20 M rows x k per 256 CUs (csrc/gemm_h2.hip: h2_config_for), so there is no
        floor of 16 clips as for self-attention; beyond that bound emage_gemm's wider tile merges a folded LayerNorm's statistics in another
        order, and the two launches stay."""
        if not (self.fuse_cross_attention and cx.h2 and not self.training and cx.dev.type == "cuda" and ops.q_attention_supported(cx.h2dt, t, tk, d, h)):
            return False
        cus = torch.cuda.get_device_properties(cx.dev).multi_processor_count
        return b * h >= cus and b * t * d < 20 * (1_000_000 * cus // 256)

    def _ln(self, cx, key, s, add=None, want_f32=False):
        """LayerNorm of a pre-norm sum (residual precision) -> _X; `add`: float32 / storage-type tensor folded in behind the norm.
        want_f32 (EMAGE_H2 mode with H2 residuals): keep a float32 twin anyway (the result is later an `add` operand)."""
        n = cx.pk.w[key]
        if isinstance(s, _S):                        # folded: nothing is launched — the consumers work on the raw sum and its statistics
            assert add is None and not want_f32
            return _X(s.img, s.img, True, ln=(s.stats, key))
        y = cx.lo(*s.shape)
        if cx.h2 and cx.h2res and not want_f32:
            ops.layernorm(cx.h2dt, s, n["g"], n["b"], 1e-5, add, None, y)
            return _X(y, y, True)
        if cx.h2:
            yf = cx.f32(*s.shape)
            ops.layernorm(cx.h2dt, s, n["g"], n["b"], 1e-5, add, yf, y)
            return _X(y, yf)
        ops.layernorm(cx.dt, s, n["g"], n["b"], 1e-5, add, None, y)
        return _X(y, y)

    def _ffn(self, cx, name, x, stats=False):
        f, _ = cx.gemm_ln(x, name + ".ff1", slope=0.0)
        return cx.gemm_s(f, name + ".ff2", x, stats)

    def _encoder_layer(self, cx, name, x, b, t, post_add=None, want_f32=False):
        """nn.TransformerEncoderLayer, post-norm, ReLU, no masks.  `fold_ln`: norm1 is folded into linear1 / the FFN's residual."""
        x = self._ln(cx, name + ".norm1", self._self_attn(cx, name, x, b, t, stats=cx.fold_ln))
        return self._ln(cx, name + ".norm2", self._ffn(cx, name, x), add=post_add, want_f32=want_f32)

    def _memory_site(self, cx, b, t, tk):
        """Whether the cross-attention sites of the two decoder stacks compute their memory K / V^T themselves (`ops.qm_attention`): the composed
        operands are packed, the site is one that `_fused_cross_attn` fuses, and the feature widths are ones the kernel takes."""
        d, h = self.config.hidden_size, spec.N_HEAD
        if not (cx.compose and self.fuse_memory_kv and cx.dev.type == "cuda" and self._fused_cross_attn(cx, b, t, tk, d, h)):
            return False
        return all(cx.pk.w[k]["cp"] <= d for k in (_BODY_KV, _FACE_KV))

    def _cross_attn(self, cx, name, x, b, t, mem):
        """Attention of x's queries over the layer's memory (`_Memory.layer`) -> att (B*T, d): one launch that computes K / V^T too (site form),
        one launch on the projected K / V^T (`_fused_cross_attn`), or the q projection and the attention."""
        d, h = self.config.hidden_size, spec.N_HEAD
        if mem.k is None:
            att = cx.lo(b * t, d)
            e, kw = self._site_operand(cx, name + ".ca.q", x, d)
            kv = cx.pk.w[mem.kv_key]
            assert kv["n"] == 2 * mem.n * d
            ops.qm_attention(cx.h2dt, x.a, e["w"], e["b"], mem.img, kv["w"], kv["b"], mem.n, mem.index, att, b, wkv_scale=kv.get("ws", 1.0), **kw)
        elif self._fused_cross_attn(cx, b, t, mem.tk, d, h):
            att = cx.lo(b * t, d)
            e, kw = self._site_operand(cx, name + ".ca.q", x, d)
            ops.q_attention(cx.h2dt, x.a, e["w"], e["b"], *mem.kv(), att, b, **kw)
        else:
            q = cx.gemm_ln(x, name + ".ca.q", want="f32")[1] if cx.h2 else cx.gemm_r(x.a, name + ".ca.q")
            att = cx.lo(b * t, d)
            ops.attention(cx.gdt, q, *mem.kv(), att, b, h, t, mem.tk, d // h)
        return att

    def _decoder_layer(self, cx, name, x, b, t, mem, post_add=None, fold_out=False):
        """nn.TransformerDecoderLayer, post-norm, ReLU, no masks.  x: _X; mem: this layer's cross-attention memory
        (`_Memory.layer`).  `fold_ln`: norm1 / norm2 are folded into the contractions around them; fold_out: norm3 too — the result is
        then an `_X` with `.ln` set, which only the next layer of the same stack can take."""
        fold = cx.fold_ln
        x = self._ln(cx, name + ".norm1", self._self_attn(cx, name, x, b, t, stats=fold))
        x = self._ln(cx, name + ".norm2", cx.gemm_s(self._cross_attn(cx, name, x, b, t, mem), name + ".ca.out", x, fold))
        return self._ln(cx, name + ".norm3", self._ffn(cx, name, x, stats=fold and fold_out and post_add is None), add=post_add)

    def _stack_memory(self, cx, stack, feats, b, tk, site):
        """The memory of decoder stack `stack` ("body" / "face") from its memory features (B*Tk, km) — the one place its form is decided.
        site (`_memory_site` for the batch that CONSUMES it): the site form, nothing is launched.  Otherwise K / V^T by `_memory_kv`: from
        the features with the composed operand (`compose_memory`), or from their projection (M:303) with the plain one.
        feats may be a `_Memory` already (features hoisted for another batch size): kept as it is, unless it is in site form and this batch
        does not take the sites — then the composed K / V launch runs here."""
        kv_key, proj, plain, n = _STACKS[stack]
        if isinstance(feats, _Memory):
            if feats.k is not None or site:
                return feats
            feats = feats.img
        if cx.compose and site:
            return _Memory(None, None, feats, kv_key, n, tk)
        if not cx.compose:
            feats, kv_key = cx.gemm(feats, proj)[0], plain
        return _Memory(*self._memory_kv(cx, kv_key, feats, b, tk, n), None, None, n, tk)

    def _memory_kv(self, cx, key, mem_lo, b, tk, n_layers):
        """Project a cross-attention memory for `n_layers` layers at once: K (B*Tk, n_layers*d) and
        V^T (B, n_layers*d, Tp)."""
        d = self.config.hidden_size
        vt = cx.vt_buffer(b, n_layers * d, tk)
        if cx.h2:                                   # float32 K / V^T for the attention kernel
            k = cx.f32(b * tk, n_layers * d)
            cx.gemm(mem_lo, key, out_f32=k, out_t=vt, t_col0=n_layers * d, t_rows=tk, want=None)
        else:
            k = cx.lo(b * tk, n_layers * d)
            cx.gemm(mem_lo, key, out=k, out_t=vt, t_col0=n_layers * d, t_rows=tk)
        return k, vt

    # ---- forward -------------------------------------------------------------------------
    def _audio_features(self, cx, audio, b, t, use_audio, fk, lane_face, lane_body, nwin=1, hop=0, win_len=None):
        """Everything that depends on the waveform only (M:275-281, 303 and the cross-attention K/V projections):
        both WavEncoders, `audio_body_motion_proj` and the 8 layers' memory K / V^T.  Returns a dict
        {memcat (B*T, audio_f+motion_f) with the face features in its first audio_f columns, body, ta}; body: the body stack's `_Memory`
        (`_stack_memory`; None without audio).
        Runs on two stream lanes of `fk`; `inference()` calls it once for ALL full windows of a batch: `audio` is then
        the whole-clip tensor, `nwin` windows of `win_len` samples every `hop` samples, b = nwin * clips sequences."""
        c = self.config
        af, mf = c.audio_f, c.motion_f
        lens = self._wav_lengths(audio.shape[1] if win_len is None else win_len)
        ta = lens[-1]
        if ta < t:
            raise RuntimeError(f"Sizes of tensors must match: audio features {ta} frames vs motion {t} frames")
        m = b * t
        feats = dict(memcat=cx.lo(m, af + mf), body=None, ta=ta)            # [audio2face | body_hint_face] (M:288)
        fused0 = self._wav_block0_fused()
        wkw = dict(wav=audio, nwin=nwin, hop=hop, win_len=win_len) if fused0 else {}
        y0 = None
        if not fused0:
            with fk.lane(lane_face):
                y0 = self._wav_first_layer(cx, audio, lens, nwin, hop, win_len)
            fk.after(lane_body, lane_face)
        with fk.lane(lane_face):
            a_face = self._wav_encoder_chain(cx, "audio_encoder_face", 0, y0, b, lens, dest=feats["memcat"][:, :af], **wkw)
            if ta > t:  # tail windows: face features trimmed to T, body features keep T' = T+1 (M:278-281, sic)
                feats["memcat"][:, :af] = a_face.view(b, ta, af)[:, :t].reshape(m, af)
            if cx.h2:   # the WavEncoder writes float32: convert the face-feature columns of the concatenation in place
                ops.cast_pad(cx.h2dt, feats["memcat"][:, :af], af, out=feats["memcat"][:, :af])
        with fk.lane(lane_body):
            a_body = self._wav_encoder_chain(cx, "audio_encoder_body", 1, y0, b, lens, **wkw)
            if use_audio:
                if cx.h2:
                    a_body = ops.cast_pad(cx.h2dt, a_body, a_body.shape[1])
                feats["body"] = self._stack_memory(cx, "body", a_body, b, ta, self._memory_site(cx, b // nwin, t, ta))
        feats["_keep"] = (y0, a_face, a_body)       # cross-lane operands stay alive until the caller's join
        return feats

    @staticmethod
    def _feats_of_clips(feats, clip0, n, t):
        """The features `_audio_features` computed for many sequences, cut to sequences [clip0, clip0 + n) of t frames (row views)."""
        body = feats["body"]
        return dict(memcat=feats["memcat"][clip0 * t:(clip0 + n) * t], ta=feats["ta"], body=None if body is None else body.clips(clip0, n))

    def _speaker_tables(self, cx, speaker_id, b, t):
        """Speaker / positional tables of a (B,T) window (M:285-286, P:341-343): they depend on the speaker ids and T
        only, so `inference()` builds them once for all full windows."""
        pk, dev, d = cx.pk, cx.dev, self.config.hidden_size
        m = b * t
        sid = speaker_id.to(dev).reshape(b, 1).expand(b, t)                 # one id per clip, broadcast over T by the kernel
        spk_body = ops.gather_rows(pk.w["spk_body"], sid, F32)              # (M,d) fp32
        spk_face = ops.gather_rows(pk.w["spk_face"], sid, F32)
        pe = pk.w["pe"][:t]
        face0, pos_spk = cx.lo(m, d), (cx.f32(m, d) if cx.h2 else cx.lo(m, d))
        if cx.h2:       # face0 enters the face decoder as operand AND residual; pos_spk is only ever added (residual precision)
            face0_r = cx.f32(m, d)
            ops.add(cx.h2dt, spk_face, pe, out_f32=face0_r, out=face0, mod_b=t)
            ops.add(F32, spk_body, pe, out=pos_spk, mod_b=t)
            face0 = _X(face0, face0_r)
        else:
            ops.add(cx.dt, spk_face, pe, out=face0, mod_b=t)                # position_embeddings(speaker_face)
            ops.add(cx.dt, spk_body, pe, out=pos_spk, mod_b=t)              # speaker_body + pe, used twice
            face0 = _X(face0, face0)
        return dict(spk_body=spk_body, face0=face0, pos_spk=pos_spk, t=t)

    def forward(self, audio, speaker_id, masked_motion, mask, use_audio=True, _audio_feats=None, _tables=None, _lean=False,
                _seed=None, _hints=None):
        """EmageAudioModel.forward (M:265-341), eval mode.  audio (B,L) fp32, speaker_id (B,1) int64,
        masked_motion / mask (B,T,337) fp32 -> dict of 8 (B,T,256) fp32 tensors.
        `_audio_feats` / `_tables` (internal): waveform-only features and speaker tables already computed by
        `inference()`; `_seed` (internal): (B, seed_frames, 337) view spliced into the first frames by the packing
        kernel (M:386-391); `_lean` (internal, `infer_codes`): skip the outputs the decode does not consume (the
        classifier of a latent-routed part, the fp32 copy of a classified part's latent); `_hints` (internal,
        `recordings.RecordingRunner`): (store_motion, store_keep, table, status) — the window's motion / mask come from
        a hint store through a device table (`ops.pack_motion_hints`); masked_motion / mask then only give the shape.
        audio / masked_motion / mask may be windows (views) of longer clip tensors: they are read in place."""
        if self.training and _audio_feats is None and _seed is None:
            # train mode (T:156-181): batch-statistics BatchNorm, dropout, outputs connected to the parameters for loss.backward()
            from . import training
            return training.train_forward(self, audio, speaker_id, masked_motion, mask, use_audio)
        c = self.config
        cx = _Ctx(self._engine(), self.h2_residual, self.fold_layernorm and c.hidden_size == _FOLD_WIDTH)
        pk = cx.pk
        dev = cx.dev
        b, t, cm = masked_motion.shape
        m = b * t
        d, mf, af = c.hidden_size, c.motion_f, c.audio_f
        if t > pk.w["pe"].shape[0]:
            raise RuntimeError(f"sequence of {t} frames exceeds the positional table ({pk.w['pe'].shape[0]})")
        if _audio_feats is None:
            audio = audio.to(device=dev, dtype=torch.float32)
            if audio.stride(1) != 1:
                audio = audio.contiguous()
        if _hints is None:
            motion3 = self._frames_view(masked_motion.to(device=dev, dtype=torch.float32))
            mask3 = self._frames_view(mask.to(device=dev, dtype=torch.float32))
            if b > 1 and motion3.stride(0) != mask3.stride(0):      # the packing kernel takes one clip stride for both
                motion3, mask3 = motion3.contiguous(), mask3.contiguous()

        out = {}
        parts = ("upper", "hands", "lower")
        others = {"upper": ("hands", "lower"), "hands": ("upper", "lower"), "lower": ("upper", "hands")}
        nf, nc = spec.N_FACE_LAYERS, spec.N_CROSS_LAYERS

        # Independent chains run on separate streams (pantomatrix_amd/streams.py).  lane 0: motion hints -> body
        # stack; lane 1: face WavEncoder -> face decoder; lane 2: body WavEncoder -> cross-attention memory.
        tables = _tables if (_tables is not None and _tables["t"] == t) else self._speaker_tables(cx, speaker_id, b, t)
        spk_body, face0, pos_spk = tables["spk_body"], tables["face0"], tables["pos_spk"]
        # which heads the caller consumes (M:403-410): classified parts (c* > 0) need cls_*, latent parts rec_*
        c_of = {"face": c.cf, "upper": c.cu, "hands": c.ch, "lower": c.cl}
        with Fork(dev, 3, self.concurrent) as fk:
            feats = _audio_feats if _audio_feats is not None else self._audio_features(cx, audio, b, t, use_audio, fk, 1, 2)
            memcat, body, ta = feats["memcat"], feats["body"], feats["ta"]
            # the stack sites compute their own K / V^T (both stacks or neither: not when the features came with projected K / V^T)
            site = use_audio and body.k is None and self._memory_site(cx, b, t, ta)

            with fk.lane(0):
                # masked motion -> spatial hints (M:267-273)
                if _hints is None:
                    x0 = ops.pack_motion(cx.dt, motion3, mask3, pk.w["mask_emb"], _rup(cm), seed=_seed)
                else:
                    store_motion, store_keep, table, status = _hints
                    x0 = ops.pack_motion_hints(cx.dt, store_motion, store_keep, table, pk.w["mask_emb"], _rup(cm), t, status, seed=_seed)
                hint, _ = _conv_encoder(cx, "motion_encoder", x0, t, spec.MOTION_ENC_LAYERS, mf, False)
                hh, _ = cx.gemm(hint, "bodyhints.fc1", slope=0.1)               # [face | body] hidden, (M, 2d)
                with ops.lockstep(self.group_gemms) as ls:                      # the two second layers: one launch
                    with ls.chain():
                        cx.gemm(hh[:, :d], "bodyhints_face.fc2", out=memcat[:, af:])
                    with ls.chain():
                        hint_body, _ = cx.gemm(hh[:, d:], "bodyhints_body.fc2")

            # face branch (M:288-294) on lane 1, once the hints (lane 0) are there
            fk.after(1, 0)
            def face_layer(i, face):
                return self._decoder_layer(cx, f"face_motion_decoder.layers.{i}", face, b, t, fmem.layer(i), fold_out=i < nf - 1)

            def cross_layer(i, x, base):
                return self._decoder_layer(cx, f"audio_motion_cross_attn.layers.{i}", x, b, t, body.layer(i),
                                           post_add=base.r if i == nc - 1 else None, fold_out=i < nc - 1)          # motion_fea + cross

            # the two decoder stacks side by side: lock step (one lane, shared launches) or two lanes
            paired = self.group_face_body and self.group_gemms and use_audio and dev.type == "cuda" and nf < nc
            with fk.lane(1):
                fmem = self._stack_memory(cx, "face", memcat, b, t, site)
                face = face0
                if not paired:
                    for i in range(nf):
                        face = face_layer(i, face)

            with fk.lane(0):
                # body branch: temporal self-attention (M:297-300)
                x = cx.gemm_x(hint_body, "moton_proj", res=pos_spk)
                x = self._encoder_layer(cx, "motion_self_encoder.layers.0", x, b, t, post_add=pos_spk,   # + speaker + pe (M:304-305)
                                        want_f32=use_audio)          # `base`: added behind the last cross-attention layer's norm
            # audio cross-attention stack (M:303-312) needs lane 2's projected memory
            first = 0
            if use_audio:
                fk.after(0, 2)
                base = x
                with fk.lane(0):
                    body = self._stack_memory(cx, "body", body, b, ta, site)
            if paired:
                fk.after(0, 1)                  # the face memory (lane 1) feeds the lock-step walk on lane 0
                pair = {}
                with fk.lane(0), ops.lockstep() as ls:
                    with ls.chain():
                        for i in range(nf):
                            face = face_layer(i, face)
                        pair["face"] = face
                    with ls.chain():
                        for i in range(nf):
                            x = cross_layer(i, x, base)
                        pair["x"] = x
                face, x, first = pair["face"], pair["x"], nf
                fk.after(1, 0)
            with fk.lane(1):
                rec_lo, out["rec_face"] = cx.gemm(face.a, "face_out_proj", want="both")
                if not (_lean and c_of["face"] == 0):
                    hc, _ = cx.gemm(rec_lo, "face_cls.fc1", slope=0.1)
                    _, out["cls_face"] = cx.gemm(hc, "face_cls.fc2", want="f32")
            if use_audio:
                with fk.lane(0):
                    for i in range(first, nc):
                        x = cross_layer(i, x, base)
            with fk.lane(0):
                # part latents (M:315-317)
                hl, _ = cx.gemm(x.a, "motion2latent.fc1", slope=0.1)             # (M, 3d)
                lat = {}
                with ops.lockstep(self.group_gemms) as ls:
                    for i, p in enumerate(parts):       # the part latents are only ever added: residual precision
                        with ls.chain():
                            lat[p] = cx.gemm_r(hl[:, i * d:(i + 1) * d], f"motion2latent_{p}.fc2")
            # refinement + heads (M:320-330): three independent chains of the same shapes on different weights.  group_gemms: walked in
            # lock step on lane 0 — every contraction of the three decoder layers and of the heads is one grouped launch (3 x 11 launches
            # -> 11).  Otherwise: "upper" stays on lane 0, "lower" takes lane 2 (idle by now), "hands" queues behind the face decoder on lane 1
            def refine_chain(p):
                tgt, mem_lo = cx.lo(m, d), cx.lo(m, d)
                if cx.h2:
                    tgt_r = cx.f32(m, d)
                    ops.add(cx.h2dt, lat[p], spk_body, out_f32=tgt_r, out=tgt)
                    tgt = _X(tgt, tgt_r)
                else:
                    ops.add(cx.dt, lat[p], spk_body, out=tgt)
                    tgt = _X(tgt, tgt)
                ops.add(cx.dt, lat[others[p][0]], lat[others[p][1]], out=mem_lo)
                name = f"body_motion_decoder_{p}.layers.0"
                mem = _Memory(*self._memory_kv(cx, name + ".ca.kv", mem_lo, b, t, 1), None, None, 1, t)
                # motion_refined + latent (M:326-328): the latent rides as the post-add of the layer's last LayerNorm (one launch less per part)
                sum_lo = self._decoder_layer(cx, name, tgt, b, t, mem.layer(0), post_add=lat[p]).a
                lean_cls = _lean and c_of[p] > 0         # decode takes the arg-max code: rec_* fp32 copy unused
                rec_lo, out[f"rec_{p}"] = cx.gemm(sum_lo, f"motion_out_proj_{p}", want="lo" if lean_cls else "both")
                if not (_lean and c_of[p] == 0):
                    hc, _ = cx.gemm(rec_lo, f"motion_cls_{p}.fc1", slope=0.1)
                    _, out[f"cls_{p}"] = cx.gemm(hc, f"motion_cls_{p}.fc2", want="f32")

            if self.group_gemms and dev.type == "cuda":
                with fk.lane(0), ops.lockstep() as ls:
                    for p in parts:
                        with ls.chain():
                            refine_chain(p)
            else:
                lane_of = {"upper": 0, "hands": 1, "lower": 2}
                fk.after(1, 0)
                fk.after(2, 0)
                for p in parts:
                    with fk.lane(lane_of[p]):
                        refine_chain(p)
        return {k: (out[k].view(b, t, -1) if out.get(k) is not None else None) for k in OUT_KEYS}


    @staticmethod
    def _frames_view(x):
        """(B, T, C) tensor whose frames are contiguous rows (strides (any, C, 1)): used as is, else made contiguous."""
        b, t, c = x.shape
        return x if (x.stride(2) == 1 and (x.stride(1) == c or t == 1)) else x.contiguous()

    # ---- inference -----------------------------------------------------------------------
    _PARTS = ("face", "upper", "hands", "lower")

    def _routes(self):
        """Latent-vs-index routing per part (M:398-410; test_emage_audio.py:34-42): "cls" = argmax(log_softmax(cls_*))
        when the part is classified (c* > 0), "lat" = the regressed latent when only l* > 0, None when neither."""
        c = self.config
        cfg = {"face": (c.lf, c.cf), "upper": (c.lu, c.cu), "hands": (c.lh, c.ch), "lower": (c.ll, c.cl)}
        return {p: ("cls" if c_ > 0 else ("lat" if l_ > 0 else None)) for p, (l_, c_) in cfg.items()}

    def _select_codes(self, net_out):
        """The keyword arguments test_emage_audio.py:34-47 builds for `EmageVQModel.decode` from the eight outputs."""
        kw = {}
        for p, route in self._routes().items():
            kw[f"{p}_latent"] = net_out.get(f"rec_{p}") if route == "lat" else None
            if route == "cls":
                logits = net_out[f"cls_{p}"]
                bsz, t, k = logits.shape
                kw[f"{p}_index"] = ops.argmax_logsoftmax(logits.reshape(bsz * t, k)).view(bsz, t)
            else:
                kw[f"{p}_index"] = None
        return kw

    def _window_codes(self, net, vq_model, codes, col0, bs, t):
        """Write one window's code indices straight into columns [col0, col0+t) of the (B, L) code buffers: arg-max of
        the classifier logits, or the nearest code of a latent-routed part (what `decode_from_latent` would compute
        from the concatenated latents — the same per-row arithmetic, so the same indices)."""
        for p, route in self._routes().items():
            if route is None:
                continue
            dst = codes[p][:, col0:col0 + t]
            src = net[f"cls_{p}" if route == "cls" else f"rec_{p}"].reshape(bs * t, -1)
            if self.health_pending is not None:      # the quantiser turns a NaN logit / latent into a valid-looking code: the caller counts
                self.health_pending.append(src.contiguous())      # them with ONE launch at the end of the batch (runtime.ClipRunner)
            elif self.health_counter is not None:
                ops.count_nonfinite(src.contiguous(), self.health_counter)
            if route == "cls":
                ops.argmax_logsoftmax(src, out=dst)
            else:
                part = getattr(vq_model, f"vq_model_{p}")
                part._nearest(_Ctx(part._engine()), src, out=dst)

    def inference(self, audio, speaker_id, vq_model, masked_motion=None, mask=None):
        """EmageAudioModel.inference (M:343-490): sliding 64-frame windows with 4 seed frames carried over
        through the VQ decode of the previous window; full windows drop their last 4 frames, an optional tail
        window of 4+remain frames is kept whole."""
        chunks = {k: [] for k in OUT_KEYS}
        for net, keep in self._windows(audio, speaker_id, vq_model, masked_motion, mask):
            for k in OUT_KEYS:
                chunks[k].append(net[k][:, :keep])
        return {k: torch.cat(chunks[k], dim=1) for k in OUT_KEYS}

    def infer_codes(self, audio, speaker_id, vq_model, masked_motion=None, mask=None):
        """The same window loop, returning what `EmageVQModel.decode` consumes instead of the eight full-length
        tensors: `{part}_index` (B, frames) int64 for every routed part (a latent-routed part — the face in the
        shipped configuration — comes back as the index of its nearest code, which is what `decode(face_latent=...)`
        would compute first).  Every kernel of a window writes its codes straight into the (B, L) code buffers and the
        seed decode reads them in place: no slicing / concatenation copies.  Used by `runtime.ClipRunner`."""
        frames = 0
        codes = None
        for net, keep in self._windows(audio, speaker_id, vq_model, masked_motion, mask, want_codes=True):
            codes = net["_codes"]
            frames += keep
        out = {k: None for k in ("face_latent", "upper_latent", "hands_latent", "lower_latent",
                                 "face_index", "upper_index", "hands_index", "lower_index")}
        if codes is not None:
            out.update({f"{p}_index": v[:, :frames] for p, v in codes.items()})
        return out

    def _seed_decode_frames(self, vq_model, t):
        """Frames the seed decode must cover: the decoder stack is 2 ResBlocks (4 convs) + vae_layer convs + 1 conv of
        kernel 3, so output frame i depends on inputs i-R..i+R with R = 5 + vae_layer; decoding the last
        seed_frames + R frames reproduces the last seed_frames outputs of the full decode exactly."""
        r = 5 + max(int(getattr(vq_model, f"vq_model_{p}").config.vae_layer) for p in ("face", "upper", "hands", "lower"))
        return min(t, self.config.seed_frames + r)

    @contextlib.contextmanager
    def collect_health(self):
        """While the block runs, `_window_codes` appends the logits / latents it takes codes from to the list this yields instead of
        counting them one by one; the caller counts them with `ops.count_nonfinite_multi` (or hands a counter to `_window_step`).  On ANY
        exit `health_pending` is None again.  Not re-entrant: a second one inside the first raises RuntimeError (the inner block would
        otherwise steal the outer one's tensors) and leaves the outer list installed."""
        if self.health_pending is not None:
            raise RuntimeError("collect_health: already collecting (the blocks do not nest)")
        self.health_pending = pending = []
        try:
            yield pending
        finally:
            self.health_pending = None

    def _window_step(self, vq_model, audio, speaker_id, motion, mask, seed, codes, col0, need_seed, counter=None, _audio_feats=None,
                     _tables=None, _hints=None):
        """ONE autoregressive window of M:380-426, for every caller (`_windows` for `infer_codes`, `recordings.RecordingRunner`,
        `streaming.StreamBatch`, tools/bench_stream.py): the lean forward of `motion` / `mask` ((B, t, 337) views) with the seed rows
        `seed` (B, seed_frames, 337) spliced in, then the window's code indices into columns [col0, col0 + t) of the (B, L) buffers `codes`,
        then — with `counter`, an int32 device counter, inside `collect_health()` — one `ops.count_nonfinite_multi` over what was collected
        so far, then, if `need_seed`, the decode of the window's last frames (M:412-418: as many as can reach the last `seed_frames`
        outputs, `_seed_decode_frames`; the whole window with `seed_only_decode` off — the same bits).
        -> the next window's seed, a (B, seed_frames, 337) view of the decode, or None."""
        b, t = motion.shape[:2]
        net = self.forward(audio, speaker_id, motion, mask, use_audio=True, _audio_feats=_audio_feats, _tables=_tables, _lean=True, _seed=seed,
                           _hints=_hints)
        self._window_codes(net, vq_model, codes, col0, b, t)
        if counter is not None and self.health_pending:
            ops.count_nonfinite_multi(list(self.health_pending), counter)
            del self.health_pending[:]
        if not need_seed:
            return None
        ts = self._seed_decode_frames(vq_model, t) if self.seed_only_decode else t
        dec = vq_model.decode(**{f"{p}_index": v[:, col0 + t - ts:col0 + t] for p, v in codes.items()})["all_motion4inference"]
        return dec[:, ts - self.config.seed_frames:]

    def _windows(self, audio, speaker_id, vq_model, masked_motion=None, mask=None, want_codes=False):
        """Generator over the autoregressive windows of M:343-470; yields (forward outputs, frames to keep).  Windows
        of the clip tensors (audio, motion, mask, code buffers) are passed to the kernels as views."""
        c = self.config
        dev = self.device
        audio = audio.to(device=dev, dtype=torch.float32)
        if audio.stride(1) != 1:
            audio = audio.contiguous()
        bs = audio.shape[0]
        length = windows.frames_of(audio.shape[1])                                              # M:345
        key = (bs, length, str(dev))
        if key not in self._templates:               # identity pose + all-ones mask (M:347-358), read-only, reused
            tmpl = windows.identity_seed(bs, length, c.pose_dims + 7, device=dev)
            self._templates = {key: (tmpl, torch.ones_like(tmpl))}
        motion, full_mask = self._templates[key]
        if masked_motion is not None:
            motion = motion.clone()
            motion[:, :masked_motion.shape[1]] = masked_motion.to(dev)
        if mask is not None:
            full_mask = full_mask.clone()
            full_mask[:, :mask.shape[1]] = mask.to(dev)
        window, pre = c.pose_length, c.seed_frames
        rounds, _remain, tail_frames = windows.split_length(length, window, pre)                 # M:364-368
        spf = windows.SPF
        hop = window - pre
        last = motion[:, :pre]                                                                   # M:370: seed of window 0
        routes = self._routes()
        codes = {p: torch.empty(bs, max(length, 1), dtype=torch.int64, device=dev) for p, r in routes.items() if r} \
            if want_codes else None

        # The waveform-only part of every full window (WavEncoders, audio projection, cross-attention K/V) does not
        # depend on the autoregressive motion state: compute it for all `rounds` windows in one set of launches
        # (rows = rounds*B sequences, read in place from the clip tensor) ahead of the sequential loop.
        hoisted = None
        open_fork = None
        tables = self._speaker_tables(_Ctx(self._engine()), speaker_id, bs, window) if rounds > 0 else None
        try:
            if rounds > 0 and self.hoist_audio:
                cx = _Ctx(self._engine())
                # Issued on the side streams the first window's forward() will use for its own lanes 1 and 2 and NOT
                # joined here: window 0's motion path (lane 0) starts at once, its face decoder and cross-attention
                # queue behind this work by stream order, and forward()'s join closes the fork.
                open_fork = Fork(dev, 3, self.concurrent)
                open_fork.__enter__()
                hoisted = self._audio_features(cx, audio, rounds * bs, window, True, open_fork, 1, 2,
                                               nwin=rounds, hop=hop * spf, win_len=window * spf)           # M:393-394
                if hoisted["ta"] != window:
                    open_fork.__exit__(None, None, None)
                    open_fork, hoisted = None, None

            def window_feats(i):
                if hoisted is None:
                    return None
                return self._feats_of_clips(hoisted, i * bs, bs, window)

            def run_window(start, end, need_seed, feats=None):
                nonlocal open_fork
                t = end - start
                a = audio[:, start * spf:start * spf + t * spf]                                      # M:393-394
                # the seed splice (M:386-391) happens inside the packing kernel: frames < pre take `last` where masked
                if want_codes:
                    seed = self._window_step(vq_model, a, speaker_id, motion[:, start:end], full_mask[:, start:end], last, codes, start,
                                             need_seed, _audio_feats=feats, _tables=tables)
                    open_fork = None                    # forward()'s own fork joined the side streams
                    return {"_codes": codes}, seed
                net = self.forward(a, speaker_id, motion[:, start:end], full_mask[:, start:end], use_audio=True,
                                   _audio_feats=feats, _tables=tables, _seed=last)
                open_fork = None
                seed = None
                if need_seed:
                    sel = self._select_codes(net)
                    # only the last `seed_frames` of the decode feed the next window (M:418): decode just the frames
                    # that can influence them (exact, see _seed_decode_frames)
                    ts = self._seed_decode_frames(vq_model, t) if self.seed_only_decode else t
                    tail_sel = {k: (None if v is None else v[:, t - ts:]) for k, v in sel.items()}
                    dec = vq_model.decode(**tail_sel)["all_motion4inference"]
                    seed = dec[:, ts - pre:]                                                         # (B, pre, 337) view
                return net, seed

            tail = tail_frames > 0
            for i in range(rounds):                                                                  # M:380-426
                start = i * hop
                # the decode only feeds the next window's seed: the reference also runs it after the last window
                # where its result is discarded; skipping that one changes no output
                net, seed = run_window(start, start + window, need_seed=(i + 1 < rounds) or tail, feats=window_feats(i))
                if seed is not None:
                    last = seed
                yield net, window - pre
            if tail:                                                                                 # M:428-470
                start = rounds * hop
                net, _ = run_window(start, start + tail_frames, need_seed=False)
                yield net, tail_frames
        finally:
            if open_fork is not None:                   # abandoned before the first window ran: join the side streams
                open_fork.__exit__(None, None, None)
