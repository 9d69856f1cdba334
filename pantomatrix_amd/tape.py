"""The model-independent half of the training forwards (`training.TrainForward`: the EMAGE graph; `training_vq.TokenizerForward`): the
reverse-mode tape, the tape-aware layer wrappers with their backward contractions (`TapeForward`), and the state every backward shares,
each with ONE owner — `ParamGrads` (gradient accumulators and what is queued for them; `discard()` is what every error path calls) and
`OperandScales` (scales, range check and cached images of the backward weight operands).  `clip_and_adam` is the tail of both trainers' step."""
from __future__ import annotations

import contextlib
import math
import weakref

import torch

from . import ops
from ._lib import F32, H2
from .modeling_emage_audio import _rup

DROPOUT_P = 0.1            # PeriodicPositionalEncoding (P:329) and nn.Transformer*Layer defaults


def _capturing(device=None):
    """True while the current stream of `device` is recording a hipGraph (no host read-back, no blocking collective result)."""
    return bool(torch.cuda.is_available() and torch.cuda.is_current_stream_capturing())


class _Masks:
    """The dropout masks of one forward: a given list (the parity tests: the reference's recorded draws), or — masks None — drawn on
    the device as they are needed (`ops.dropout_mask`: Philox keyed by rng = (seed, step, first mask id); step may be a device scalar).
    needs: how many masks the forward consumes (for the message of a list that runs out)."""

    def __init__(self, masks, dev, rng=None, lazy=True, needs=None):
        self.masks, self.i, self.dev, self.rng, self.lazy, self.needs = (None if masks is None else list(masks)), 0, dev, rng, lazy, needs
        if masks is None and rng is None:
            raise RuntimeError("train-mode forward: pass dropout_masks or an rng (seed, step, first mask id)")

    def consumed_all(self):
        return self.masks is None or self.i == len(self.masks)

    def take(self, shape, lazy=False):
        """The next mask of the forward, of logical shape `shape`.  lazy (device-drawn masks only): the caller consumes it through
        `ops.mul_add` alone, which draws the mask inside its kernel — return the key (`ops.PhiloxMask`) instead of a tensor."""
        if self.masks is None:
            seed, step, base = self.rng
            if lazy and self.lazy and shape[-1] % 4 == 0:
                self.i += 1
                return ops.PhiloxMask(shape, DROPOUT_P, seed, base + self.i - 1, step, self.dev)
            m = torch.empty(tuple(shape), dtype=torch.float32, device=self.dev)
            ops.dropout_mask(m, DROPOUT_P, seed, base + self.i, step)
            self.i += 1
            return m
        if self.i >= len(self.masks):
            raise RuntimeError(f"dropout_masks: {len(self.masks)} masks given, the forward needs {self.needs}")
        m = self.masks[self.i]
        self.i += 1
        if tuple(m.shape) != tuple(shape):
            raise RuntimeError(f"dropout mask {self.i - 1}: shape {tuple(m.shape)}, the reference draws {tuple(shape)} here")
        return m.to(device=self.dev, dtype=torch.float32).contiguous()


class _Token:
    """Stands for a logical (rows, cols) tensor that exists only in pieces (a projection whose V columns are stored transposed)."""

    def __init__(self, shape):
        self.shape = shape


def _accumulate(dst, g, out=None):
    """out (default dst) = dst + g on fp32 (rows, cols) views: emage_add where its 16-byte granularity allows, torch otherwise
    (the 337-column motion rows)."""
    out = dst if out is None else out
    if g.shape[1] % 4 == 0 and all(t.stride(0) % 4 == 0 and t.data_ptr() % 8 == 0 for t in (dst, g, out)):
        ops.add(F32, dst, g, out=out)
    else:
        torch.add(dst, g, out=out)


class _Tape:
    """Reverse-mode bookkeeping of one forward: backward closures in launch order, gradient buffers keyed by the forward tensor
    (or token) they belong to, column-slice views routed into their parent's buffer.  Gradients are fp32 (rows, cols).
    Memory: a gradient buffer lives from its first contribution until the node that PRODUCED its tensor has run (every consumer of a
    tensor runs before its producer in reverse order, and a tensor has one producer); a closure — and with it the activations it saved —
    is dropped as soon as it has run.  So the live set shrinks as the backward walks instead of doubling until its end."""

    def __init__(self, dev):
        self.dev, self.nodes, self.g, self.views, self.keep, self.kids, self.pos = dev, [], {}, {}, {}, {}, -1
        self._fetched = None            # ids whose gradient the running node has taken (dropped behind the node)
        self.pinned = set()

    def node(self, fn):
        self.nodes.append(fn)

    def view(self, parent, view, c0, written=False):
        """`view` = parent[:, c0:c0 + width] takes part in the forward under its own identity.  written: the view is the OUTPUT of a node
        (the parent is assembled in pieces, so it has several producers): its gradient buffer then stays until the tape is dropped."""
        self.views[id(view)] = (parent, c0, view.shape[1])
        self.keep[id(view)] = view                       # ids are keys: the objects must stay alive while their entries exist
        self.kids.setdefault(id(parent), []).append(id(view))
        if written:
            self.pinned.add(id(parent))

    def buffer(self, t, zero=True):
        """The zero-initialised, tape-owned gradient buffer of `t` (created on first use).  zero=False: the caller (and its siblings)
        OVERWRITE every column block before anyone reads the buffer — the attention backward's dQ / dK / dV blocks of a projection."""
        e = self.g.get(id(t))
        if e is None:
            alloc = torch.zeros if zero else torch.empty
            e = [alloc(tuple(t.shape), dtype=torch.float32, device=self.dev), True]
            self.g[id(t)] = e
            self.keep[id(t)] = t
        elif not e[1]:
            e[0], e[1] = e[0].clone(), True
        return e[0]

    def add(self, t, g, cols=None):
        """grad(t)[:, :cols] += g.  The first gradient of a tensor is kept by reference (never modified in place afterwards)."""
        if id(t) in self.views:
            parent, c0, n = self.views[id(t)]
            dst = self.buffer(parent)[:, c0:c0 + (n if cols is None else cols)]
            _accumulate(dst, g)
            return
        e = self.g.get(id(t))
        if cols is not None and cols != t.shape[1]:
            dst = self.buffer(t)[:, :cols]
            _accumulate(dst, g)
        elif e is None:
            self.g[id(t)] = [g, False]
            self.keep[id(t)] = t
        elif e[1]:
            _accumulate(e[0], g)
        else:
            s = torch.empty(tuple(e[0].shape), dtype=torch.float32, device=self.dev)
            _accumulate(e[0], g, out=s)
            e[0], e[1] = s, True

    def add_through(self, t, make, cols=None):
        """grad(t)[:, :cols] += c for a contribution that a contraction produces: `make(prev)` launches it and returns `c` (prev None) or
        `prev + c` as a NEW tensor (prev: the gradient so far, handed to the launch as its float32 residual — the add rides in the
        epilogue instead of being a launch of its own; the same bits: fl(prev + fl(c)))."""
        e = None if id(t) in self.views or (cols is not None and cols != t.shape[1]) else self.g.get(id(t))
        if e is None:
            self.add(t, make(None), cols)
        else:
            e[0], e[1] = make(e[0]), True

    def get(self, t):
        if id(t) in self.views:                          # a column block of its parent's gradient
            parent, c0, n = self.views[id(t)]
            e = self.g.get(id(parent))
            return None if e is None else e[0][:, c0:c0 + n]
        e = self.g.get(id(t))
        if e is None:
            return None
        if self._fetched is not None:
            self._fetched.append(id(t))
        return e[0]

    def _drop(self, i):
        if i in self.pinned:
            return
        self.g.pop(i, None)
        self.keep.pop(i, None)
        for v in self.kids.pop(i, ()):
            self.views.pop(v, None)
            self.keep.pop(v, None)

    def run(self, progress=None, base=0):
        """Run the recorded closures in reverse; `pos` counts the executed nodes (what `ParamGrads.rows` stamps a parameter's
        last contribution with); progress(pos) is called behind each node (the overlapped gradient exchange hangs on it).  base: position
        of the first node (a tape run as the continuation of another one: the step-shared WavEncoder pass behind the third backward)."""
        self.pos = base - 1
        if progress is not None and base == 0:
            progress(-1)
        k = 0
        while self.nodes:
            fn = self.nodes.pop()
            self.pos = base + k
            self._fetched = []
            try:
                fn()
            finally:
                fetched, self._fetched = self._fetched, None
            del fn
            for i in fetched:
                self._drop(i)
            if progress is not None:
                progress(base + k)
            k += 1


class ParamGrads:
    """The parameter gradients of a training forward: name -> fp32 accumulator, shared by the forwards of a step, and what is still on
    its way into them.  Contributions are QUEUED and applied in batches (`flush`: one multi-tensor add for up to 256 of them instead of one
    small launch each, ~1 200 per step; the column reductions' finalize steps 64 to a launch, `ops.FinalizeQueue`); every element still
    receives its contributions one by one in issue order, so the sums are the same bits.  `discard()` is the one way to drop what a
    backward that died had queued."""
    MAX_QUEUED, MAX_BYTES = 256, 96 << 20

    def __init__(self, param, position):
        """param(name) -> the parameter (the shape of a lazily created accumulator); position() -> the running tape node (`touch`)."""
        self._param, self._position = param, position
        self.acc = {}                   # name -> gradient accumulator (`current()` is the flushed view of it)
        self.views = None               # name -> preallocated fp32 gradient tensor (views of the exchange buckets, training.Trainer)
        self.touch = None               # a dict (set by `Trainer` while it learns its exchange schedule): name -> tape position of the parameter's last contribution
        self.finalize = ops.FinalizeQueue()                      # queued finalize steps of the bias / affine-gradient reductions
        self._dst, self._src, self._spans, self._bytes = [], [], {}, 0      # queued `add` contributions

    def current(self):
        """name -> fp32 gradient accumulated so far (queued contributions applied first: reading is always consistent)."""
        self.flush()
        return self.acc

    def start(self, acc):
        """Accumulate into the dict `acc` from here on; contributions queued for the previous accumulators are applied to them first."""
        self.flush()
        self.acc = acc

    def pending(self):
        """(queued adds, queued finalize entries)."""
        return len(self._dst), len(self.finalize.entries)

    def rows(self, name, rows):
        """The rows `rows` of parameter `name`'s gradient accumulator (the exchange bucket's view under a `Trainer`) as the destination of
        one more contribution: a queued contribution to overlapping rows is applied first; the tape position is stamped."""
        full = self.acc.get(name)
        if full is None:
            full = self.views[name] if self.views is not None else torch.zeros_like(self._param(name), dtype=torch.float32)
            self.acc[name] = full
        n0 = full.shape[0] if full.dim() else 1
        lo, hi = (0 if rows.start is None else rows.start), (n0 if rows.stop is None else rows.stop)
        spans = self._spans.get(name)
        if spans is not None and any(lo < b and a < hi for a, b in spans):
            self.flush()
        if self.touch is not None:
            self.touch[name] = self._position()
        return full[rows], (lo, hi)

    def add(self, name, rows, g):
        """grad(name)[rows] += g — parameter-sized accumulation across the forwards of a step, queued."""
        dst, span = self.rows(name, rows)
        g = g.reshape(dst.shape)
        self._spans.setdefault(name, []).append(span)
        self._dst.append(dst)
        self._src.append(g)
        self._bytes += g.numel() * 4
        if len(self._dst) >= self.MAX_QUEUED or self._bytes >= self.MAX_BYTES:
            self.flush()

    def add_colsum(self, name, rows, x, y=None, defer=True):
        """grad(name)[rows] += column sums of x (* y): the bias / affine gradients, accumulated by the reduction's own finalize launch
        (defer: queued with the others)."""
        dst, _span = self.rows(name, rows)
        ops.col_sum(x, y, out=dst, accumulate=True, defer=self.finalize if defer else None)

    def flush(self):
        """Apply the queued contributions (call before anything reads or exchanges the accumulators)."""
        self.finalize.flush()             # the queued finalize steps of the column reductions (bias / affine gradients)
        if self._dst:
            # ONE pair that is not dense with equal strides (the convolutions' weight gradients arrive as permuted (Cout, taps, Cin) views) sends the
            # WHOLE multi-tensor add down torch's one-launch-per-tensor path (~440 launches per step): those pairs go in a call of their own.  The
            # queued destinations never overlap (`rows` flushes first), so the order between the two calls does not matter
            plain = [d.stride() == g.stride() and d.is_contiguous() for d, g in zip(self._dst, self._src)]
            for want in (True, False):
                dst = [d for d, ok in zip(self._dst, plain) if ok == want]
                if dst:
                    torch._foreach_add_(dst, [g for g, ok in zip(self._src, plain) if ok == want])
        self._dst, self._src, self._spans, self._bytes = [], [], {}, 0

    def discard(self):
        """Drop every queued add and every queued finalize entry (a backward that died mid-walk: its float64 partials would otherwise
        land in the NEXT flush).  What has been applied stays in the accumulators: their owner decides (`Trainer` zeroes its buckets)."""
        self.finalize.entries = []
        self._dst, self._src, self._spans, self._bytes = [], [], {}, 0

    @contextlib.contextmanager
    def alone(self):
        """The gradients of ONE backward alone: inside, contributions go to a fresh dict (yielded; complete when the block ends); behind
        it the caller's accumulators are back.  An exception discards what the block had queued."""
        saved = self.current()
        self.acc = own = {}
        try:
            yield own
            self.flush()
        except BaseException:
            self.discard()
            raise
        finally:
            self.acc = saved


class OperandScales:
    """The weight operands of the split-fp16 backward contractions: per key a power-of-two scale, chosen once and checked on the device
    from then on, and the scaled EMAGE_H2 image (transposed Linear weights, flattened / flipped convolution filters), built once per
    forward — once per step inside `keep_images()`, where the weights do not move between the forwards."""

    def __init__(self):
        self._keep = False
        self.reset()

    def reset(self):
        """Forget scales, images and the range flag: the next use chooses afresh from the current weights."""
        self._scale, self._images = {}, {}
        self.range_flag = None          # int32 device counter: operands whose cached scale no longer fits
        self._pending, self._seen = [], set()

    def scale(self, key, w):
        """Power-of-two scale of a backward weight operand: chosen at the first use of `key` (one read-back: max |w| into [2^11, 2^12)) and
        kept, so that later steps — and a captured step — convert without a host round trip.  Every later use checks ON THE DEVICE that
        max |w| * scale is still inside [2^10, 2^14) (`ops.f16_scale_out_of_range`; the fp16 hi plane overflows at 2^16) and counts a
        miss in `range_flag`, which `Trainer` reads with the losses and answers by re-deriving the scales (`reset`)."""
        ws = self._scale.get(key)
        if ws is None:
            mx = float(w.abs().max())
            ws = self._scale[key] = 2.0 ** (11 - math.floor(math.log2(mx))) if mx > 0 and math.isfinite(mx) else 1.0
        elif w.numel() and key not in self._seen:       # once per key and step, all keys in a few launches (`flush_checks`)
            self._seen.add(key)
            self._pending.append((w, ws))
        return ws

    def image(self, key, build):
        """The cached (image, scale) of `key`; build() makes it on a miss."""
        hit = self._images.get(key)
        if hit is None:
            hit = self._images[key] = build()
        return hit

    def flush_checks(self, new_step=False):
        """Fold the operands queued by `scale` into `range_flag`; new_step: forget which keys this step has seen."""
        if self._pending:
            ws, scales = zip(*self._pending)
            self._pending = []
            bad = ops.f16_scales_out_of_range(list(ws), list(scales))
            self.range_flag = bad if self.range_flag is None else self.range_flag + bad
        if new_step:
            self._seen = set()

    def new_forward(self):
        """A forward starts: its weights may differ from the last one's, so the images go — unless a step keeps them."""
        if not self._keep:
            self._images = {}

    @contextlib.contextmanager
    def keep_images(self):
        """One optimisation step: the parameters move at its END, so one set of images, built from scratch, serves all its forwards."""
        self._images, self._keep = {}, True
        try:
            yield
        finally:
            self._images, self._keep = {}, False


class TapeForward:
    """What the train-mode forwards share: parameter lookup, the tape-aware Linear / Conv1d(k=3) / add / dropout / LayerNorm wrappers
    (each launches the forward op and, when a tape is attached, records its backward), the backward contractions, and the delegates to
    the two owners (`grads`, `scales`).  A subclass writes `__call__` and `backward`."""

    def __init__(self, model):
        if model.precision == "bf16":
            raise ValueError("the training forward runs in the fp32-storage precisions (f16x3 / fp32)")
        self.model = model
        # f16x3 precision: the backward contractions run as split-fp16 MFMA on pre-split (EMAGE_H2) operands — gradients pre-scaled by
        # a power of two so that their fp16 planes stay normal (the loss-scaling of mixed-precision training, undone exactly in the
        # GEMM epilogue); fp32 precision keeps the exact-fp32 MFMA contractions
        self.h2_backward = model.precision == "f16x3"
        self.grad_scale = 1024.0
        self.conv_backward_rows = 1 << 17                 # output rows per piece of a long convolution's backward (_conv_backward_h2)
        self.fuse_grad_adds = True      # a Linear's input gradient is added to what its input has collected so far by the contraction's own epilogue (A/B switch; same bits)
        self.direct_conv_dx = True      # stride-1 convolutions: the input gradient as ONE implicit-GEMM convolution of dY (A/B switch; False: dcol = dY W + col2im)
        self.accumulate_dw = True       # Linear weight gradients are added into the gradient rows by their contraction (A/B switch; False: a temporary + a queued add)
        self.defer_finalize = True      # bias / affine-gradient reductions end in batched finalize launches (`ops.FinalizeQueue`; A/B switch: False = one each)
        self.splitk_workspace_bytes = 32 << 20            # scratch of the two-pass split-K weight-gradient contractions (emage_gemm_ws: K-slices as planes, added
        self._splitk_buf = None                           # in slice order — bit-reproducible gradients); 0: the fp32-atomic form of emage_gemm
        self.tape = None
        me = weakref.proxy(self)        # (the owner must not keep this object — and the buckets its accumulators view — alive in a cycle)
        self.grads = ParamGrads(lambda name: me._param(name), lambda: me.tape.pos)
        self.scales = OperandScales()
        self._grad_rows, self._param_grad, self.flush_param_grads = self.grads.rows, self.grads.add, self.grads.flush
        self.flush_range_checks = self.scales.flush_checks
        self._pcache = None

    def _begin_forward(self, cx, tape):
        """Start of a forward on the operand context `cx`: a fresh tape (or none), parameters read afresh, images per `OperandScales`."""
        self.tape = _Tape(cx.dev) if tape else None
        self._cx = cx
        self._pcache = None
        self.scales.new_forward()

    def _splitk_ws(self, dev=None):
        """The workspace of the weight-gradient contractions (one buffer per trainer: the launches of a step run in stream order)."""
        if not self.splitk_workspace_bytes:
            return None
        dev = self.model.device if dev is None else dev
        if self._splitk_buf is None or self._splitk_buf.device != dev or self._splitk_buf.numel() * 4 != self.splitk_workspace_bytes:
            self._splitk_buf = torch.empty(self.splitk_workspace_bytes // 4, dtype=torch.float32, device=dev)
        return self._splitk_buf

    # ---- parameters, their gradients (`ParamGrads`) and operand scales (`OperandScales`) ------------------------------------------------
    def _params(self):
        """name -> detached parameter / buffer view, built once per forward (walking the module tree per lookup costs more than
        the launches it feeds)."""
        if self._pcache is None:
            dev = self.model.device
            self._pcache = {k: v.detach().to(dev) for k, v in self.model._flat_params().items()}
        return self._pcache

    def _param(self, name):
        return self._params()[name]

    def parameters_moved(self):
        """The parameters were updated behind this object's back (Adam through raw pointers, a graph replay): read them afresh."""
        self._pcache = None

    # thin delegates to the owners (with `_grad_rows`, `_param_grad`, `flush_param_grads`, `flush_range_checks` of `__init__`): the names callers use
    param_grads = property(lambda self: self.grads.current(), lambda self, acc: self.grads.start(acc))       # reading and assigning flush first
    grad_views = property(lambda self: self.grads.views, lambda self, views: setattr(self.grads, "views", views))
    range_flag = property(lambda self: self.scales.range_flag)

    def reset_scales(self):
        """Forget the cached operand scales (backward weight operands here, the forward's packed operands in the model): the next
        forward chooses them afresh from the current weights."""
        self.scales.reset()
        self.model.invalidate_packed(reset_scales=True)
        self._pcache = None

    # ---- Conv1d backward ------------------------------------------------------------------------------------------------------------
    def _conv_backward(self, cx, x, cin, origins, dy, taps, stride, pad, lin, lout, nseq, need_dx):
        """Conv1d backward on channels-last rows through emage_gemm (exact fp32): x (nseq*lin, >= cin) the layer input, dy (nseq*lout, N)
        the gradient of its pre-activation output; origins = [(weight name, bias name)] of the convolutions stacked along N.
        Accumulates the parameter gradients; returns dx (nseq*lin, cin) when asked."""
        ws = [self._param(wn).float() for wn, _ in origins]                      # (Cout_i, Cin, k)
        n = sum(w.shape[0] for w in ws)
        m = dy.shape[0]
        mp = _rup(m)
        if self.h2_backward:
            return self._conv_backward_h2(cx, x, cin, origins, ws, dy, n, m, mp, taps, stride, pad, lin, lout, nseq, need_dx)
        dy_t = torch.zeros(n, mp, dtype=torch.float32, device=cx.dev)
        ops.transpose(dy, dy_t)
        col_t = ops.im2col_t(x, cin, taps, stride, pad, lin, lout, nseq, mp)     # (taps*cin, mp)
        kc = taps * cin
        dw = torch.empty(n, _rup(kc, 4), dtype=torch.float32, device=cx.dev)[:, :kc]          # 16-byte row pitch for emage_gemm's stores
        ops.gemm(F32, dy_t, col_t, None, None, None, dw, None, None, n=kc, cp=mp)
        self._conv_param_grads(origins, ws, dw, ops.col_sum(dy), taps, cin)
        if not need_dx:
            return None
        wflat = torch.cat([w.permute(0, 2, 1).reshape(w.shape[0], taps * cin) for w in ws], 0).contiguous()        # (N, taps*cin), taps major
        np_ = _rup(n)
        if np_ != n:                           # the contraction length is a multiple of 64: zero channels (the tokenizers' 106 / 78 / 180 / 61 / 240-wide layers)
            dy = torch.nn.functional.pad(dy, (0, np_ - n))
            wflat = torch.nn.functional.pad(wflat, (0, 0, 0, np_ - n))
        dcol = torch.empty(m, _rup(kc, 4), dtype=torch.float32, device=cx.dev)[:, :kc]
        ops.gemm(F32, dy, ops.transpose(wflat), None, None, None, dcol, None, None, n=kc, cp=np_)
        return ops.col2im(dcol, cin, taps, stride, pad, lin, lout, nseq)

    def _conv_param_grads(self, origins, ws, dw, db, taps, cin):
        """Hand dW (N, taps*Cin; taps major) and db (N) of convolutions stacked along N to their parameters."""
        r0 = 0
        for (wn, bn), w in zip(origins, ws):
            rows = w.shape[0]
            self._param_grad(wn, slice(None), dw[r0:r0 + rows].reshape(rows, taps, cin).permute(0, 2, 1))
            self._param_grad(bn, slice(None), db[r0:r0 + rows])
            r0 += rows

    def _conv_backward_h2(self, cx, x, cin, origins, ws, dy, n, m, mp, taps, stride, pad, lin, lout, nseq, need_dx):
        """`_conv_backward` with both contractions as split-fp16 MFMA on EMAGE_H2 operands: dW = (gs dY)^T im2col(X) with the im2col matrix
        written directly as an H2 image, dcol = (gs dY) W with the flattened weights converted once per forward.  Long inputs (the first
        WavEncoder blocks: 56 clips x 6 827 positions) are walked in pieces of whole sequences of about `conv_backward_rows` output rows, so
        the im2col image, the transposed dY and dcol exist for one piece at a time (0.5 GB instead of 1.5 GB each); dW is summed over the pieces."""
        gs = self.grad_scale
        kc = taps * cin
        per = max(1, self.conv_backward_rows // max(lout, 1))
        pieces = [(s0, min(s0 + per, nseq)) for s0 in range(0, nseq, per)]
        w_t = wsc = None
        np_ = _rup(n)
        # stride-1 'same' convolutions (every conv2 of the WavEncoder blocks, the motion encoder): dX is itself a convolution of dY with the
        # flipped, transposed filters — ONE implicit-GEMM launch per piece writing dX, instead of dcol = dY W (M x taps*Cin float32: 1.5 GB for
        # the first block at 56 clips) + col2im
        direct = need_dx and self.direct_conv_dx and stride == 1 and lin == lout and 2 * pad == taps - 1 and cin % 8 == 0
        if direct:
            key = ("conv^T",) + tuple(wn for wn, _ in origins)

            def build():
                wcat = torch.cat(ws, 0) if len(ws) > 1 else ws[0]                                                      # (N, Cin, k)
                wrev = torch.nn.functional.pad(wcat.flip(2).permute(1, 2, 0), (0, np_ - n)).reshape(cin, taps * np_).contiguous()   # [ci][k-1-tap][co], co padded
                wsc = self.scales.scale(key, wcat)
                return ops.h2_cast(wrev, taps * np_, scale=wsc / 16.0), wsc
            w_t, wsc = self.scales.image(key, build)
        elif need_dx:
            key = ("conv",) + tuple(wn for wn, _ in origins)

            def build():
                wflat = torch.cat([w.permute(0, 2, 1).reshape(w.shape[0], kc) for w in ws], 0).contiguous()          # (N, taps*cin), taps major
                wsc = self.scales.scale(key, wflat)
                return ops.h2_cast(wflat, np_, scale=wsc / 16.0, transpose=True), wsc                                  # (taps*cin, rup64(N))
            w_t, wsc = self.scales.image(key, build)
        dw = dx = None
        for s0, s1 in pieces:
            whole = len(pieces) == 1
            xs = x if whole else x[s0 * lin:s1 * lin]
            dys = dy if whole else dy[s0 * lout:s1 * lout]
            ms = (s1 - s0) * lout
            mps = _rup(ms)
            dy_t = ops.h2_cast(dys, mps, scale=gs, transpose=True)                          # (N, mps)
            col_t = ops.im2col_t_h2(xs, cin, taps, stride, pad, lin, lout, s1 - s0, mps)    # (taps*cin, mps)
            dwp = torch.empty(n, _rup(kc, 4), dtype=torch.float32, device=cx.dev)[:, :kc]
            ops.gemm(H2, dy_t, col_t, None, None, None, None, dwp, None, n=kc, cp=mps, w_scale=16.0, a_scale=16.0 * gs, workspace=self._splitk_ws(cx.dev))
            del col_t, dy_t
            dw = dwp if dw is None else dw.add_(dwp)
            if direct:
                dy_h = ops.h2_cast(dys, np_, scale=gs)
                if dx is None:
                    dx = torch.empty(nseq * lin, cin, dtype=torch.float32, device=cx.dev)
                ops.gemm(H2, dy_h, w_t, None, None, None, None, dx if whole else dx[s0 * lin:s1 * lin], None, n=cin, cp=np_, taps=taps, stride=1, pad=taps - 1 - pad,
                         lin=lout, lout=lin, m=(s1 - s0) * lin, w_scale=wsc, a_scale=16.0 * gs)
                del dy_h
            elif need_dx:
                dy_h = ops.h2_cast(dys, np_, scale=gs)
                dcol = torch.empty(ms, _rup(kc, 4), dtype=torch.float32, device=cx.dev)[:, :kc]
                ops.gemm(H2, dy_h, w_t, None, None, None, None, dcol, None, n=kc, cp=np_, w_scale=wsc, a_scale=16.0 * gs, workspace=self._splitk_ws(cx.dev))
                del dy_h
                part = ops.col2im(dcol, cin, taps, stride, pad, lin, lout, s1 - s0)
                del dcol
                if whole:
                    dx = part
                else:
                    if dx is None:
                        dx = torch.empty(nseq * lin, cin, dtype=torch.float32, device=cx.dev)
                    dx[s0 * lin:s1 * lin].copy_(part)
                del part
        self._conv_param_grads(origins, ws, dw, ops.col_sum(dy), taps, cin)
        return dx

    # ---- Conv1d(k=3) + LeakyReLU + ResBlock stacks (VQEncoderV5 / V6, VQDecoderV5: P:178-261), tape-aware --------------------------------
    def _conv3(self, cx, x, key, t, b, cin, slope=None, res=None, need_dx=True):
        """y (M, rup64(n)) = act(conv3(x) + bias) (+ res); columns [n, rup64(n)) are zero.  need_dx False: x is the network's input."""
        n = cx.pk.w[key]["n"]
        y, _ = cx.conv3(x, key, t, slope=slope, res=res, n_store=_rup(n))
        if self.tape is not None:
            def bw():
                g = self.tape.get(y)
                if g is None:
                    return
                if res is not None:
                    self.tape.add(res, g)
                yv = y
                if g.shape[1] != n:                      # a width that is not a multiple of 64: the padding columns carry no gradient
                    g, yv = g[:, :n].contiguous(), y[:, :n]
                dpre = g if slope is None else ops.act_backward(g, yv, slope)
                dx = self._conv_backward(cx, x, cin, [(key + ".weight", key + ".bias")], dpre, 3, 1, 1, t, t, b, need_dx)
                if need_dx:
                    self.tape.add(x, dx, cols=cin)
            self.tape.node(bw)
        return y

    def _conv_encoder(self, cx, prefix, x0, t, b, cin0, n_layer, need_dx=True):
        """VQEncoderV5 / V6 (P:189-235): n_layer x [conv + LeakyReLU(0.2) + ResBlock].  need_dx False: no gradient for x0."""
        h, cin = x0, cin0
        for i in range(n_layer):
            p = f"{prefix}.main.{3 * i}"
            h = self._conv3(cx, h, p, t, b, cin, slope=0.2, need_dx=need_dx or i > 0)
            cin = cx.pk.w[p]["n"]
            r = self._conv3(cx, h, f"{prefix}.main.{3 * i + 2}.model.0", t, b, cin, slope=0.2)
            h = self._conv3(cx, r, f"{prefix}.main.{3 * i + 2}.model.2", t, b, cin, res=h)
        return h

    def _conv_decoder(self, cx, prefix, z, t, b, length, n_layer):
        """VQDecoderV5 (P:237-261): two ResBlocks, n_layer x [conv + LeakyReLU(0.2)], a bare conv -> (M, rup64(out_dim))."""
        h, cin = z, length
        for i in range(2):
            r = self._conv3(cx, h, f"{prefix}.main.{i}.model.0", t, b, cin, slope=0.2)
            h = self._conv3(cx, r, f"{prefix}.main.{i}.model.2", t, b, cin, res=h)
        for i in range(n_layer):
            key = f"{prefix}.main.{2 + 2 * i}"
            h = self._conv3(cx, h, key, t, b, cin, slope=0.2)
            cin = cx.pk.w[key]["n"]
        return self._conv3(cx, h, f"{prefix}.main.{2 + 2 * n_layer}", t, b, cin)

    # ---- Linear -----------------------------------------------------------------------------------------------------------------------
    def _lin(self, cx, x, key, slope=None, out=None, need_dx=True):
        """y = act(x W^T + b) through emage_gemm (one fp32 output used both as the next operand and as the result)."""
        y, _ = cx.gemm(x, key, slope=slope, out=out)
        if self.tape is not None:
            self.tape.node(lambda: self._lin_backward(cx, x, key, slope, y, y, need_dx))
        return y

    def _lin_kv(self, cx, x, key, n_first, t_rows, b):
        """A projection whose last columns are emitted transposed (V^T for emage_attention): returns (first n_first columns as
        rows, the V^T buffer, a token standing for the logical (M, N) output in the tape)."""
        n = cx.pk.w[key]["n"]
        first = cx.lo(x.shape[0], n_first)
        vt = cx.vt_buffer(b, n - n_first, t_rows)
        cx.gemm(x, key, out=first, out_t=vt, t_col0=n_first, t_rows=t_rows)
        token = _Token((x.shape[0], n))
        if self.tape is not None:
            self.tape.node(lambda: self._lin_backward(cx, x, key, None, token, None, True))
        return first, vt, token

    def _lin_backward(self, cx, x, key, slope, y_id, y, need_dx):
        tape = self.tape
        dy = tape.get(y_id)
        if dy is None:
            return
        ent = cx.pk.w[key]
        n, k = ent["n"], ent["k_real"]
        m = dy.shape[0]
        if dy.shape[1] != n or dy.stride(1) != 1:
            raise RuntimeError(f"{key}: gradient of shape {tuple(dy.shape)} for an output of {n} columns")
        if self.h2_backward:
            self._lin_backward_h2(cx, x, key, dy, y if slope is not None else None, slope, n, k, m, need_dx)
            return
        dpre = dy if slope is None else ops.act_backward(dy, y, slope)
        w32 = torch.cat([self._param(wn)[rs] for wn, _bn, rs in cx.pk.origin[key]], 0).float().contiguous()            # (N, K)
        mp = _rup(m)
        dpre_t = torch.zeros(n, mp, dtype=torch.float32, device=cx.dev)
        ops.transpose(dpre, dpre_t)
        x_t = torch.zeros(k, mp, dtype=torch.float32, device=cx.dev)
        ops.transpose(x[:, :k], x_t)
        dw = torch.empty(n, k, dtype=torch.float32, device=cx.dev)
        ops.gemm(F32, dpre_t, x_t, None, None, None, dw, None, None, n=k, cp=mp)                                          # dW = dpre^T x
        self._lin_param_grads(cx, key, dw, dpre)
        if need_dx:
            np_ = _rup(n)
            if np_ != n:
                raise RuntimeError(f"{key}: {n} output columns (not a multiple of 64) — pad before the backward contraction")
            w_t = ops.transpose(w32)                                                                                    # (K, N)
            dx = torch.empty(m, k, dtype=torch.float32, device=cx.dev)
            ops.gemm(F32, dpre, w_t, None, None, None, dx, None, None, n=k, cp=n)                                        # dX = dpre W
            tape.add(x, dx, cols=k)

    def _lin_param_grads(self, cx, key, dw, dpre):
        """Hand dW (N, K) and the bias gradient (column sums of dpre) of the packed Linear `key` to the parameters it stacks."""
        origin = cx.pk.origin[key]
        if len(origin) == 1:                              # the usual case: the reduction's finalize adds into the gradient rows itself
            wn, bn, rs = origin[0]
            self._param_grad(wn, rs, dw)
            self.grads.add_colsum(bn, rs, dpre, defer=self.defer_finalize)
            return
        db = ops.col_sum(dpre)
        r0 = 0
        for wn, bn, rs in origin:
            rows = rs.stop - rs.start
            self._param_grad(wn, rs, dw[r0:r0 + rows])
            self._param_grad(bn, rs, db[r0:r0 + rows])
            r0 += rows

    def _weight_t_h2(self, cx, key, n, k):
        """The transposed weight of a Linear as an EMAGE_H2 operand, (K, rup64(N)) holding w * w_scale: (image, w_scale); built once per
        forward and key, scale from `OperandScales.scale`."""
        def build():
            rows = [self._param(wn)[rs] for wn, _bn, rs in cx.pk.origin[key]]
            w32 = (torch.cat(rows, 0) if len(rows) > 1 else rows[0]).float().contiguous()                                # (N, K); one source: no copy
            ws = self.scales.scale(key, w32)
            return ops.h2_cast(w32, _rup(n), scale=ws / 16.0, transpose=True), ws     # h2 images carry a fixed x16: the rest of the scale goes in front
        return self.scales.image(key, build)

    def _lin_backward_h2(self, cx, x, key, dy, y, slope, n, k, m, need_dx):
        """dW = dpre^T x, db = colsum(dpre), dX = dpre W as split-fp16 MFMA contractions (emage_gemm, EMAGE_H2).  dpre = dy through the
        activation's backward (y: the layer's saved output, None = no activation).  ONE pass over dy (`ops.grad_prep`) yields both
        gradient operands — pre-scaled by `grad_scale`, undone by the GEMM's output scale — and the bias gradient, which the reduction's
        finalize launch adds straight into the parameter's gradient rows when the packed key holds one Linear."""
        gs = self.grad_scale
        mp = _rup(m)
        origin = cx.pk.origin[key]
        single = len(origin) == 1
        bias_dst = self._grad_rows(origin[0][1], origin[0][2])[0] if single else None
        dpre_h, dpre_t, db = ops.grad_prep(dy, y, 0.0 if slope is None else slope, gs, n_store=_rup(n) if need_dx else None, m_store=mp,
                                           bias_grad=bias_dst, accumulate=single,                # (M, rup64(N)), (N, mp)
                                           defer=self.grads.finalize if (single and self.defer_finalize) else None)
        x_t = ops.h2_cast(x[:, :k], mp, scale=1.0, transpose=True)                    # (K, mp)
        wdst = self._grad_rows(origin[0][0], origin[0][2])[0] if single else None
        if self.accumulate_dw and wdst is not None and wdst.dim() == 2 and wdst.stride(1) == 1 and wdst.stride(0) % 4 == 0 and wdst.data_ptr() % 16 == 0:
            # dW added by the contraction itself (res == out_f32: the epilogue's residual add in place, or split-K atomics onto the contents)
            ops.gemm(H2, dpre_t, x_t, None, None, wdst, None, wdst, None, n=k, cp=mp, w_scale=16.0, a_scale=16.0 * gs, workspace=self._splitk_ws())
        else:
            dw = torch.empty(n, k, dtype=torch.float32, device=cx.dev)
            ops.gemm(H2, dpre_t, x_t, None, None, None, None, dw, None, n=k, cp=mp, w_scale=16.0, a_scale=16.0 * gs, workspace=self._splitk_ws(cx.dev))
            r0 = 0
            for wn, bn, rs in origin:
                rows = rs.stop - rs.start
                self._param_grad(wn, rs, dw[r0:r0 + rows])
                r0 += rows
        if not single:
            r0 = 0
            for wn, bn, rs in origin:
                rows = rs.stop - rs.start
                self._param_grad(bn, rs, db[r0:r0 + rows])
                r0 += rows
        if need_dx:
            w_t, ws = self._weight_t_h2(cx, key, n, k)

            def make(prev):                            # prev: the gradient x has collected so far (its residual path) — added by this launch's epilogue
                dx = torch.empty(m, k, dtype=torch.float32, device=cx.dev)
                if prev is not None and not (self.fuse_grad_adds and prev.shape == dx.shape and prev.stride(1) == 1 and prev.stride(0) % 4 == 0 and prev.data_ptr() % 16 == 0):
                    ops.gemm(H2, dpre_h, w_t, None, None, None, None, dx, None, n=k, cp=_rup(n), w_scale=ws, a_scale=16.0 * gs, workspace=self._splitk_ws(cx.dev))
                    out = torch.empty_like(dx)
                    _accumulate(prev, dx, out=out)
                    return out
                ops.gemm(H2, dpre_h, w_t, None, None, prev, None, dx, None, n=k, cp=_rup(n), w_scale=ws, a_scale=16.0 * gs, workspace=self._splitk_ws(cx.dev))
                return dx
            self.tape.add_through(x, make, cols=k)

    # ---- element-wise pieces ------------------------------------------------------------------------------------------------------------
    def _add(self, cx, a, bb, mod_b=0, grad_b=True):
        out = cx.lo(*a.shape)
        ops.add(cx.dt, a, bb, out=out, mod_b=mod_b)
        if self.tape is not None:
            def bw():
                g = self.tape.get(out)
                if g is None:
                    return
                self.tape.add(a, g)
                if grad_b and not mod_b:
                    self.tape.add(bb, g)
            self.tape.node(bw)
        return out

    def _mul_add(self, a, mask, res=None, t_rows=0):
        out = ops.mul_add(a, mask, res, mask_t_rows=t_rows)
        if self.tape is not None:
            def bw():
                g = self.tape.get(out)
                if g is None:
                    return
                self.tape.add(a, ops.mul_add(g, mask, None, mask_t_rows=t_rows))
                if res is not None:
                    self.tape.add(res, g)
            self.tape.node(bw)
        return out

    def _layernorm(self, cx, key, s_in):
        n = cx.pk.w[key]
        y = cx.lo(*s_in.shape)
        ops.layernorm(cx.dt, s_in, n["g"], n["b"], 1e-5, None, None, y)
        if self.tape is not None:
            def bw():
                g = self.tape.get(y)
                if g is None:
                    return
                dg, _ = self._grad_rows(key + ".weight", slice(None))
                db, _ = self._grad_rows(key + ".bias", slice(None))
                dx, _, _ = ops.layernorm_backward(s_in, n["g"], g, dgamma=dg, dbeta=db, defer=self.grads.finalize if self.defer_finalize else None)      # d gamma / d beta += inside
                self.tape.add(s_in, dx)
            self.tape.node(bw)
        return y


# ======================================================================================
# the tail of an optimisation step: clip by the global norm, then Adam
# ======================================================================================
def _check_max_norm(value):
    if value is None:
        return None
    value = float(value)
    if not value > 0:
        raise ValueError("max_grad_norm must be positive (None: no clipping)")
    return value


def _param_grad_norms(gn, names, pre_scale):
    if gn is None:
        raise RuntimeError("param_grad_norms: no step has run with max_grad_norm / track_grad_norm set")
    return {n: pre_scale * v ** 0.5 for n, v in zip(names, gn.tensor_sumsq.tolist())}


def clip_and_adam(table, step, lr, betas, eps, weight_decay, skip, max_norm=None, track=False, world=1):
    """`ops.grad_norm` over the Adam table when clipping (max_norm) or tracking — the global norm of the gradient SUM times 1 / world = the
    norm of the average; the coefficient rides into Adam on the device — then ONE `ops.adam_multi` that also clears the gradients and
    honours the skip word.  step: an int or the device-side counter.  -> the launch's `ops.GradNorm`, None when neither is on."""
    norm, clip = None, {}
    if max_norm is not None or track:
        norm = ops.grad_norm(table, pre_scale=1.0 / world, max_norm=max_norm)
        if max_norm is not None:
            clip = dict(grad_scale_dev=norm.coef)
    ops.adam_multi(table, step, lr, betas[0], betas[1], eps, weight_decay, grad_scale=1.0 / world, zero_grad=True, skip=skip, **clip)
    return norm
