"""Gestures from LIVE audio: a fixed number of slots, each one session of `EmageAudioModel.inference` (M:343-470) whose waveform arrives in
chunks while it runs, all slots advancing in lock step — one `forward` at B = slots per tick, one captured graph for the life of the batch.
Sessions open, push PCM, receive frames and close at different times; the other slots keep running and nothing is captured again.

The stream computes what the offline pass (`recordings.RecordingRunner`, the reference's `inference()` + `decode(get_global_motion=True)`)
computes for the same audio.  Three rules make that so (DESIGN.md derives them):

1. WHEN a window may run.  Window i reads samples [60 i 533, 60 i 533 + 64 * 533) but runs only once the session holds
   `samples_for_frames(60 i + 64)` samples: only then is n * 30 // 16000 >= 60 i + 64 for every total n the session may be closed at, so the
   offline `rounds = (L - 4) // 60` contains window i as a FULL window.  (34112 + 31980 i samples would run windows the reference treats as
   part of a tail.)  The two counts drift apart by 20 samples a window; the audio ring is sized for it.
2. HOW FAR emission lags.  Every convolution of kernel 3 widens the receptive field by a frame: a part decoder reaches 5 + vae_layer frames
   either side, the translation path (lower decoder, global encoder, global decoder) R = (5 + L_lower) + (5 + 4 L_global).  A frame is
   emitted once codes up to frame + R exist — one lag for poses, expressions and translation — decoded from the segment of the last
   60 + 2 R codes, whose rows nearer than R to an edge that is not a true end of the stream are discarded.  At frame 0 the segment starts at
   frame 0 (the reference zero-pads there); the true end is `close()`'s, decoded at its true length.
3. The translation CONTINUES.  `emage_stream_emit` applies the step of `emage_velocity_to_position` (csrc/vel_step.h, shared) from the
   position carried per slot, so the streamed translation is one scan over the whole velocity sequence, bit for bit.

A batch built with ``audio_inputs=(AudioInput(48000, 1, "s16"), ...)`` takes each session's PCM as its source produces it — any rate, 1-8
channels, 16 / 24 / 32-bit integer or float32 — and resamples it inside the tick (`ops.stream_push_resample`), with a fourth rule:

4. WHICH samples a slot holds.  The offline front end (`ops.audio_resample`) computes y[m] = sum_k h[m down + half - k up] x[k]; output m
   reads frames up to (m down + half) // up, so after n frames the first `available(n)` = ceil((n up - half) / down) outputs are FINAL —
   they no longer depend on what follows, nor on where the pushes were cut — and only those count as `pushed`.  The 10-20 outputs behind
   them wait for more input or for `end()`, which computes them against zeros: the offline right edge.  The ring then holds, bit for
   bit, the offline kernel's samples, and rules 1-3 apply to them unchanged.

A batch built with ``motion_hints=True`` takes MOTION HINTS from its sessions while they run (`open(motion=True)`, `push_motion`,
`end_motion`) — keyframes, a body part tracked by a headset and controllers, a pose to hold: the `masked_motion` / `mask` of the reference's
`inference()` (M:343-359), as `recordings.RecordingRunner(hints=True)` honours them offline — with a fifth rule:

5. WHICH hint frames a window needs.  A hinted session's concatenated output equals, code for code, the offline hinted pass
   (`RecordingSet(masked_motion=[m], mask=[k])` through `RecordingRunner(hints=True)`: the reference's B = 1 call), m / k being the
   prefix of motion and mask rows the session pushed before it ended its hints.  Window i packs frames [60 i, 60 i + 64) (M:380-391): a
   hint frame f is read by window (f - 4) // 60 as one of its frames 4 .. 63, and, when f % 60 < 4 and f >= 60, by window f // 60 too, as a
   seed frame — there mask == 0 makes the hint win over the decoded seed (M:386-390).  So window i of a session whose hints are open runs
   only once rule 1 holds AND the session holds hint frames up to 60 i + 64 or has ended its hints (`end_motion()`): only then does the
   window read what the offline pass reads, whatever is pushed later.  Frames behind the end of the hints count as template and masked (the
   reference's prefix semantics, M:352-359); window 0's seed is the first four rows of the hinted motion over the identity template
   (M:379), whatever their mask says.  Until then `Session.ready` is False and `Session.waiting` says "motion".

* ``StreamBatch``  the slots, their device state and the tick;
* ``Session``      one live stream: `push(pcm)`, `end()`, `push_motion(...)`, `end_motion()`, `close()`;
* ``Emitted``      what a session receives: poses (n, 165), expressions (n, 100), trans (n, 3), codes {part: (n,) int64}."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import audio, ops, synthetic
from ._lib import nonfinite_error
from .audio import available                            # rule 4: the outputs that are final after n input frames
from .recordings import HINT_LD, _hint_template
from .windows import MODEL_SR, SEED_DIMS, SPF, frames_of, identity_seed, split_length

STATUS_TEXT = ops.STREAM_STATUS_TEXT
_SAMPLE_BYTES = {"s16": 2, "s24": 3, "s32": 4, "f32": 4}
_PUSH_DTYPES = {"s16": np.int16, "s24": np.uint8, "s32": np.int32, "f32": np.float32}


class Emitted(NamedTuple):
    poses: np.ndarray
    expressions: np.ndarray
    trans: np.ndarray
    codes: dict


def decode_radius(vq_model):
    """(R_part, R) of rule 2: frames either side a code can reach in the poses / in anything the decode returns."""
    r_part = 5 + max(int(getattr(vq_model, f"vq_model_{p}").config.vae_layer) for p in ("face", "upper", "hands", "lower"))
    r_trans = (5 + int(vq_model.vq_model_lower.config.vae_layer)) + (5 + 4 * int(vq_model.global_motion.config.vae_layer))
    return r_part, max(r_part, r_trans)


def window_need(i, window=64, hop=60):
    """Rule 1: samples a session must hold before window i runs."""
    return synthetic.samples_for_frames(hop * i + window)


def tail_of(n_samples, pre=4, hop=60):
    """(rounds, tail frames) of a recording of `n_samples` samples: M:345, M:364-368; the tail window has pre + remain frames when
    remain > pre (M:428-431), else there is none (0)."""
    total = frames_of(n_samples)
    if total <= pre:
        return 0, 0
    rounds, _remain, tail = split_length(total, hop + pre, pre)
    return rounds, tail


class Session:
    """One live stream in one slot of a `StreamBatch`.  pushed: 16 kHz samples the slot holds; windows: full windows run; emitted: frames
    handed out; frames_in: raw frames accepted (= pushed, unless the batch resamples: then pushed counts the FINAL outputs, rule 4)."""

    def __init__(self, batch, slot, speaker_id, fmt=None, motion=False):
        self.batch, self.slot, self.speaker_id = batch, slot, speaker_id
        self.pushed = self.windows = self.emitted = self.frames_in = 0
        self.closed = self.ended = False
        self.fmt = fmt                                      # row of the batch's declared audio inputs (None: the 16 kHz path)
        self._staged = []                                   # host chunks not on the device yet
        self._sent = self._written = 0                      # resampling batch: frames uploaded / outputs written to the ring so far
        # motion hints (rule 5).  hint_frames: hint frames pushed; hint_frames_unused: after close(), those beyond the frames produced
        self.motion, self.hints_ended = bool(motion), not motion
        self.hint_frames = self.hint_frames_unused = 0
        self._hint_staged, self._hint_sent = [], 0          # (form, motion rows or None, mask rows) not on the device yet / frames uploaded

    def push(self, pcm):
        self.batch._push(self, pcm)

    def push_motion(self, motion=None, mask=None, *, poses=None, trans=None, contact=None):
        """Append n consecutive hint frames behind those already pushed (a session opened with motion=True).  Packed form: motion (n, 337)
        float32 in the model's layout (55 x rot6d | trans | contact).  Tracker form: poses (n, 165) axis-angle with trans (n, 3) and contact
        (n, 4), missing ones zero — converted on the device, the bits of `ops.axis_angle_to_rot6d`.  mask (n, 337) of exactly 0 / 1, 1 =
        generate, 0 = given (`RecordingSet`'s rule; anything else raises ValueError); None: all ones.  A mask with neither motion nor poses
        hints the identity template.  Hints wait on the host for the next tick; the two forms do not mix among the frames of one tick.  A
        push that would make the slot hold more than 60 * windows + hint_rows hint frames raises."""
        self.batch._push_motion(self, motion, mask, poses, trans, contact)

    def end_motion(self):
        """No more hints: the frames behind those pushed are generated freely (rule 5).  Idempotent; `close()` calls it."""
        self.batch._end_motion(self)

    def end(self):
        """No more input.  In a resampling batch the outputs held back for lack of later frames (rule 4) are released — computed against
        zeros, the offline right edge — with the next launch; that can make one more full window ready.  Idempotent; `close()` calls it."""
        self.batch._end(self)

    def close(self):
        return self.batch._close(self)

    @property
    def waiting(self):
        """What the session's next full window waits for: "audio" (rule 1), "motion" (rule 5: the audio is there, hint frames up to
        60 windows + 64 are not and the hints have not ended), or None (it runs at the next tick; a closed session waits for nothing)."""
        if self.closed:
            return None
        if self.pushed < window_need(self.windows, self.batch.window, self.batch.hop):
            return "audio"
        if not self.hints_ended and self.hint_frames < self.batch.hop * self.windows + self.batch.window:
            return "motion"
        return None

    @property
    def ready(self):
        return not self.closed and self.waiting is None


class StreamBatch:
    """`slots` sessions in lock step.

    Device state per slot: an fp32 audio ring of `ring_len` samples (absolute sample a of the session lives at a mod ring_len; samples behind
    the next window's start may be overwritten), a ring of the last `ring_codes` codes per routed part, the 4 seed rows the next window
    starts from, the translation carry, the speaker id.  `step()` uploads the PCM staged since the last tick and a table row per slot
    (`ops.stream_table`), runs the tick — push, windows, `forward` at B = slots, codes, seed decode, commit, segment decode, emit — as ONE
    graph replay (use_graph=False: eagerly), and downloads the output rows.  Slots that are not ready run on zero audio; `commit` drops what
    they compute and leaves their state bit for bit.

    audio_format: "f32" or "s16" (decoded x * 2^-15 on the device) — the dtype `push` takes.  max_seconds: the longest session; with
    max_push (the most samples a session may hold beyond what its next window needs) it sizes the ring: a push that does not fit raises.
    Weights are fixed for the life of the batch: `step()` raises once the model's version stamp has moved.

    audio_inputs: None, or the `audio.AudioInput`s (rate, channels, sample format) sessions of this batch may push — fixed here, their filters
    uploaded once.  The tick's first launch is then `ops.stream_push_resample`: each slot's raw PCM is decoded, down-mixed and resampled to
    16 kHz on the device, filter state carried per slot, so that the ring holds bit for bit what `ops.audio_resample` gives for the
    session's whole PCM (rule 4); `open(audio_input=...)` picks a session's format, `push` takes (n, channels) frames of it (packed 24-bit:
    (n, 3 * channels) uint8).  `audio_format` is not used then; max_push and max_seconds stay in 16 kHz samples.

    motion_hints: False — nothing is allocated for hints and the tick is the launch sequence of a batch without the argument.  True — every
    slot owns a hint ring, `hint_ring_motion` (slots, hint_rows + 4, 344) float32 / `hint_ring_keep` uint8 with
    hint_rows = 60 * ceil((64 + max_hint_push) / 60): hint frame f of a session lives at row f % hint_rows and rows hint_rows .. + 3 mirror
    rows 0 .. 3, so window i is the 64 contiguous rows from (60 i) % hint_rows.  The tick has one more launch, `ops.stream_push_hints`,
    which scatters the hint frames staged since the last tick into the rings (tracker-form frames converted on the way), copies a session's
    frames 0 .. 3 into its seed rows and writes the (slots, 2) table through which the forward's packing launch
    (`ops.pack_motion_hints`, as in `RecordingRunner(hints=True)`) reads every slot's window — {0, 0}, a window without hints, for slots
    that are not ready and for sessions opened without `motion=True`, whose bits are those of a batch without hints.  max_hint_push: the most
    hint frames a session may hold beyond the 64 its next window needs; the pinned staging buffer is sized for it at construction."""

    def __init__(self, model, vq_model, slots=8, audio_format="f32", max_seconds=3600, use_graph=True, max_push=3 * MODEL_SR, audio_inputs=None,
                 motion_hints=False, max_hint_push=90):
        dev = model.device
        model._require_device(dev)                          # an MI355X: there is no CPU path (the host tests lift this check over stand-in ops)
        on_gpu = dev.type == "cuda"
        c = model.config
        if int(c.pose_length) != 64 or int(c.seed_frames) != 4:
            raise ValueError("StreamBatch: the model must have pose_length 64 and seed_frames 4")
        if audio_format not in ("f32", "s16"):
            raise ValueError("StreamBatch: audio_format must be 'f32' or 's16'")
        if int(slots) <= 0 or int(max_push) <= 0 or max_seconds <= 0:
            raise ValueError("StreamBatch: slots, max_push and max_seconds must be positive")
        self.model, self.vq, self.device, self.slots = model, vq_model, dev, int(slots)
        self.window, self.pre = 64, 4
        self.hop = self.window - self.pre
        self.r_part, self.lag = decode_radius(vq_model)
        self.seg_len = self.hop + 2 * self.lag
        self.ring_codes = -(-self.seg_len // self.hop) * self.hop          # a multiple of the hop: an append never wraps
        self.max_samples = int(max_seconds * MODEL_SR)
        i_max = max((frames_of(self.max_samples) - self.pre) // self.hop, 1)
        self.ring_len = window_need(0) + 20 * i_max + int(max_push)        # rule 1's drift + the largest backlog
        self.audio_dtype = torch.float32 if audio_format == "f32" else torch.int16
        self.parts = [p for p, r in model._routes().items() if r]
        s, n_p = self.slots, len(self.parts)
        self.audio_inputs = None if audio_inputs is None else tuple(audio_inputs)
        staged_len = s * self.ring_len
        if self.audio_inputs is not None:
            self.formats, taps, self.hist_len = ops.stream_formats(self.audio_inputs, MODEL_SR)      # ValueError for what the kernel does not take
            self.ratios = [audio.rate_ratio(a.rate, MODEL_SR) for a in self.audio_inputs]
            self.frame_bytes = [a.channels * _SAMPLE_BYTES[a.fmt] for a in self.audio_inputs]
            # the most a slot can have staged: the frames behind ring_len outputs plus those held back, in the format with the most bytes per
            # 16 kHz sample; every slot's chunk starts on a 16-byte boundary
            worst = max(((self.ring_len * down + audio.stream_half(up, down)) // up + 2) * fb for (up, down), fb in zip(self.ratios, self.frame_bytes))
            self.audio_dtype, staged_len = torch.uint8, s * (-(-worst // 16) * 16)
            self.taps = torch.from_numpy(taps).to(dev)
            self.history = torch.zeros(s, 2, self.hist_len, device=dev)        # per slot two sides: a push reads one and writes the other
            self.hist_side = [0] * s
            self.rs_table = torch.zeros(s, ops.STREAM_RS_WORDS, dtype=torch.int32, device=dev)
            self.rs_table_host = torch.zeros(s, ops.STREAM_RS_WORDS, dtype=torch.int32, pin_memory=on_gpu)
        # ---- device state ----
        self.ring = torch.zeros(s, self.ring_len, device=dev)
        self.code_ring = torch.zeros(n_p, s, self.ring_codes, dtype=torch.int64, device=dev)
        self.seeds = identity_seed(s).to(dev)
        self.carry = torch.zeros(s, 3, device=dev)
        self.speaker_id = torch.zeros(s, 1, dtype=torch.long, device=dev)
        # ---- per tick ----
        self.staged = torch.zeros(staged_len, dtype=self.audio_dtype, device=dev)
        self.staged_host = torch.zeros(staged_len, dtype=self.audio_dtype, pin_memory=on_gpu)
        self.table = torch.zeros(s, ops.STREAM_WORDS, dtype=torch.int32, device=dev)
        self.table_host = torch.zeros(s, ops.STREAM_WORDS, dtype=torch.int32, pin_memory=on_gpu)
        self.win_audio = torch.zeros(s, self.window * SPF, device=dev)
        self.win_codes = torch.zeros(n_p, s, self.window, dtype=torch.int64, device=dev)
        self.segment = torch.zeros(n_p, s, self.seg_len, dtype=torch.int64, device=dev)
        self.tmpl_motion = identity_seed(s, self.window).to(dev)           # identity pose + all-ones mask (M:347-358), read-only
        self.tmpl_mask = torch.ones_like(self.tmpl_motion)
        self._ident = identity_seed(1)[0]
        self.motion_hints = bool(motion_hints)
        if self.motion_hints:
            if int(max_hint_push) <= 0:
                raise ValueError("StreamBatch: max_hint_push must be positive")
            self.hint_rows = self.hop * -(-(self.window + int(max_hint_push)) // self.hop)
            rows = self.hint_rows + self.pre
            self.hint_ring_motion = _hint_template(s * rows).view(s, rows, HINT_LD).to(dev)      # the template's contents: a row nobody pushed is no hint
            self.hint_ring_keep = torch.ones(s, rows, HINT_LD, dtype=torch.uint8, device=dev)
            self._hint_store = (self.hint_ring_motion.view(s * rows, HINT_LD)[:, :SEED_DIMS], self.hint_ring_keep.view(s * rows, HINT_LD)[:, :SEED_DIMS])
            self.window_table = torch.zeros(s, 2, dtype=torch.int64, device=dev)
            self.hint_table = torch.zeros(s, ops.STREAM_HINT_WORDS, dtype=torch.int32, device=dev)
            self.hint_table_host = torch.zeros(s, ops.STREAM_HINT_WORDS, dtype=torch.int32, pin_memory=on_gpu)
            # the most a slot can have staged: a full ring of frames in the wider (packed) form
            hint_bytes = s * ops.stream_hint_chunk_bytes(self.hint_rows, ops.STREAM_HINT_PACKED)
            self.hint_staged = torch.zeros(hint_bytes, dtype=torch.uint8, device=dev)
            self.hint_staged_host = torch.zeros(hint_bytes, dtype=torch.uint8, pin_memory=on_gpu)
            self.hint_bytes_staged = 0                      # bytes the last tick uploaded (tools/bench_stream.py)
        # the output rows and the two flags [non-finite values, status word] in ONE buffer: one device-to-host copy per tick
        self.out, self.out_views = self._output_buffer(s, self.hop, dev, False)
        self.out_host, self.host_views = self._output_buffer(s, self.hop, torch.device("cpu"), on_gpu)
        self.nonfinite, self.status = self.out_views["flags"][0:1], self.out_views["flags"][1:2]
        self.sessions = [None] * s
        self.precision = model.precision
        self.graph, self._operands = None, None
        self.ticks = 0
        self._upload([None] * s)
        self._tick()                                                        # no slot ready: packs weights, warms the allocator, validates shapes
        if on_gpu:
            torch.cuda.synchronize(dev)
        self._stamp = self._version_stamp()
        if use_graph and on_gpu:
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
                self._tick()
            if self._version_stamp() != self._stamp:
                raise RuntimeError("StreamBatch: capturing the tick re-packed the models' operands")
        # what the tick's launches read: alive as long as the batch, whatever becomes of the models
        self._operands = (model._packed, [m._packed for m in vq_model._models()], dict(vq_model._templates))

    def _output_buffer(self, s, rows, dev, pinned):
        n_p = len(self.parts)
        sizes = (("poses", s * rows * 165, torch.float32), ("expressions", s * rows * 100, torch.float32), ("trans", s * rows * 3, torch.float32),
                 ("flags", 2, torch.int32), ("codes", s * rows * n_p, torch.int64))
        f32_bytes = sum(n for _k, n, _d in sizes[:4]) * 4
        pad = -f32_bytes % 8
        buf = torch.zeros(f32_bytes + pad + sizes[4][1] * 8, dtype=torch.uint8, device=dev, pin_memory=pinned)
        views, lo = {}, 0
        for k, n, dt in sizes:
            if k == "codes":
                lo += pad
            nbytes = n * (8 if dt == torch.int64 else 4)
            views[k] = buf[lo:lo + nbytes].view(dt)
            lo += nbytes
        views["poses"], views["expressions"] = views["poses"].view(s, rows, 165), views["expressions"].view(s, rows, 100)
        views["trans"], views["codes"] = views["trans"].view(s, rows, 3), views["codes"].view(s, rows, n_p)
        return buf, views

    def _version_stamp(self):
        return (self.model._version_stamp(),) + tuple(m._version_stamp() for m in self.vq._models())

    # ---- sessions -----------------------------------------------------------------------------------------------------------------------
    def open(self, speaker_id=0, seed=None, ref_trans=None, audio_input=None, motion=False):
        """A new session in the lowest free slot (raises when there is none).  seed (4, 337) / ref_trans (3,): as `RecordingSet` seeds a
        recording; None: identity pose, zero translation (test_emage_audio.py).  audio_input: in a batch built with `audio_inputs`, the one
        of them this session pushes (None: the first).  The session starts with an empty filter history, whatever the slot held before.
        motion=True (a batch built with motion_hints=True): a hinted session — it pushes motion hints (`push_motion`) and its windows wait
        for them (rule 5) until `end_motion()`.  Its seed is the first four frames of its hints over the identity (M:379), so `seed` and
        motion=True exclude each other, as `seeds` and `masked_motion` do in `RecordingSet`."""
        if motion and seed is not None:
            raise ValueError("StreamBatch.open: pass `seed` or motion=True, not both (the seed is the first four frames of the hints, M:379)")
        if motion and not self.motion_hints:
            raise ValueError("StreamBatch.open: motion=True needs a batch built with motion_hints=True")
        free = [k for k, s in enumerate(self.sessions) if s is None]
        if not free:
            raise RuntimeError(f"StreamBatch: all {self.slots} slots are in use")
        if not 0 <= int(speaker_id) < int(self.model.config.speaker_dims):
            raise ValueError(f"StreamBatch.open: speaker id {speaker_id} outside [0, {int(self.model.config.speaker_dims)})")
        fmt = None
        if self.audio_inputs is None:
            if audio_input is not None:
                raise ValueError("StreamBatch.open: audio_input needs a batch built with audio_inputs=(...)")
        elif audio_input is None:
            fmt = 0
        elif audio_input in self.audio_inputs:
            fmt = self.audio_inputs.index(audio_input)
        else:
            raise ValueError(f"StreamBatch.open: {audio_input} is not one of the batch's declared audio inputs {self.audio_inputs}")
        k = free[0]
        seed = self._ident if seed is None else torch.as_tensor(seed, dtype=torch.float32)
        ref_trans = torch.zeros(3) if ref_trans is None else torch.as_tensor(ref_trans, dtype=torch.float32)
        if tuple(seed.shape) != (self.pre, SEED_DIMS) or tuple(ref_trans.shape) != (3,):
            raise ValueError(f"StreamBatch.open: seed {tuple(seed.shape)} / ref_trans {tuple(ref_trans.shape)}, expected (4, {SEED_DIMS}) / (3,)")
        self.seeds[k].copy_(seed)                           # stream-ordered copies into fixed addresses: the next replay reads them
        self.carry[k].copy_(ref_trans)
        self.speaker_id[k].fill_(int(speaker_id))
        self.sessions[k] = s = Session(self, k, int(speaker_id), fmt, motion)
        return s

    def _fits(self, s, pushed, n):
        """Raises unless a session that then holds `pushed` 16 kHz samples fits max_seconds and its slot's ring."""
        if pushed > self.max_samples:
            raise ValueError(f"Session.push: {pushed} samples exceed max_seconds ({self.max_samples} samples)")
        if pushed - self.hop * SPF * s.windows > self.ring_len:
            raise ValueError(f"Session.push: {n} samples do not fit: the slot would hold {pushed - self.hop * SPF * s.windows} samples behind its "
                             f"next window, its ring {self.ring_len} (call step(), or build the batch with a larger max_push)")

    def _push_frames(self, s, a):
        """`_push` of a resampling batch: `a` holds frames of the session's declared format."""
        inp, (up, down) = self.audio_inputs[s.fmt], self.ratios[s.fmt]
        width = inp.channels * (3 if inp.fmt == "s24" else 1)
        if a.ndim == 1 and width == 1:
            a = a[:, None]
        if a.ndim != 2 or a.shape[1] != width or a.dtype != _PUSH_DTYPES[inp.fmt]:
            raise ValueError(f"Session.push: this session takes {inp}: (n, {width}) {np.dtype(_PUSH_DTYPES[inp.fmt]).name} frames, not {a.shape} {a.dtype}")
        n = int(a.shape[0])
        # the ring and max_seconds are checked against what `end()` would release too, so that ending a session never overflows either
        self._fits(s, audio.out_length(s.frames_in + n, up, down), n)
        if n:
            s._staged.append(np.ascontiguousarray(a).view(np.uint8).reshape(-1))
            s.frames_in += n
            s.pushed = available(s.frames_in, up, down)

    def _end(self, s):
        if s.closed:
            raise RuntimeError("Session.end: the session is closed")
        if not s.ended and s.fmt is not None:
            s.pushed = audio.out_length(s.frames_in, *self.ratios[s.fmt])
        s.ended = True

    def _push(self, s, pcm):
        if s.closed:
            raise RuntimeError("Session.push: the session is closed")
        if s.ended:
            raise RuntimeError("Session.push: the session's input has ended")
        a = pcm.detach().cpu().numpy() if torch.is_tensor(pcm) else np.asarray(pcm)
        if s.fmt is not None:
            return self._push_frames(s, a)
        if a.ndim != 1:
            raise ValueError(f"Session.push: a 1-D chunk of samples, not {a.shape}")
        if self.audio_dtype == torch.int16:
            if a.dtype != np.int16:
                raise ValueError(f"Session.push: this batch takes int16 PCM (audio_format='s16'), not {a.dtype}")
        elif a.dtype == np.int16:
            a = a.astype(np.float32) * np.float32(1.0 / 32768.0)
        elif a.dtype != np.float32:
            raise ValueError(f"Session.push: float32 or int16 samples, not {a.dtype}")
        n = int(a.shape[0])
        self._fits(s, s.pushed + n, n)
        if n:
            s._staged.append(np.ascontiguousarray(a))
            s.pushed += n
            s.frames_in += n

    # ---- motion hints (rule 5) ----------------------------------------------------------------------------------------------------------------
    def _push_motion(self, s, motion, mask, poses, trans, contact):
        if s.closed:
            raise RuntimeError("Session.push_motion: the session is closed")
        if not s.motion:
            raise RuntimeError("Session.push_motion: the session was opened without motion=True")
        if s.hints_ended:
            raise RuntimeError("Session.push_motion: the session's hints have ended")
        if motion is not None and poses is not None:
            raise ValueError("Session.push_motion: pass `motion` (packed, (n, 337)) or `poses` (tracker, (n, 165)), not both")
        if poses is None and (trans is not None or contact is not None):
            raise ValueError("Session.push_motion: `trans` / `contact` belong to the tracker form: pass `poses` with them")

        def rows_of(name, a, width):
            if a is None:
                return None
            a = np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a)
            if a.ndim != 2 or a.shape[1] != width:
                raise ValueError(f"Session.push_motion: {name} must be (n, {width}), got {a.shape}")
            return a
        given = [(nm, rows_of(nm, a, w)) for nm, a, w in (("motion", motion, SEED_DIMS), ("mask", mask, SEED_DIMS), ("poses", poses, 165),
                                                           ("trans", trans, 3), ("contact", contact, 4)) if a is not None]
        if not given:
            raise ValueError("Session.push_motion: nothing to push: pass motion, poses or mask")
        n = int(given[0][1].shape[0])
        if any(a.shape[0] != n for _nm, a in given):
            raise ValueError(f"Session.push_motion: the arrays disagree on the number of frames: {[(nm, a.shape[0]) for nm, a in given]}")
        given = dict(given)
        if "mask" in given and not ((given["mask"] == 0) | (given["mask"] == 1)).all():       # RecordingSet's rule (np.isin costs ten times this)
            raise ValueError("Session.push_motion: mask must hold exactly 0 (given) and 1 (generate)")
        if s.hint_frames + n > self.hop * s.windows + self.hint_rows:
            raise ValueError(f"Session.push_motion: {n} frames do not fit: the slot would hold {s.hint_frames + n - self.hop * s.windows} hint frames "
                             f"behind its next window, its ring {self.hint_rows} (call step(), or build the batch with a larger max_hint_push)")
        form, data = None, None
        if "motion" in given:
            form, data = ops.STREAM_HINT_PACKED, np.array(given["motion"], dtype=np.float32)      # a copy: the frames wait here until the next tick
        elif "poses" in given:
            form, data = ops.STREAM_HINT_TRACKER, np.zeros((n, ops.STREAM_HINT_WIDTHS[ops.STREAM_HINT_TRACKER]), dtype=np.float32)
            data[:, :165] = given["poses"]
            if "trans" in given:
                data[:, 165:168] = given["trans"]
            if "contact" in given:
                data[:, 168:172] = given["contact"]
        if form is not None and any(f is not None and f != form for f, _d, _k in s._hint_staged):
            raise ValueError("Session.push_motion: packed and tracker frames do not mix among the frames of one tick; call step() between them")
        if n:
            keep = np.ones((n, SEED_DIMS), np.uint8) if "mask" not in given else given["mask"].astype(np.uint8)
            s._hint_staged.append((form, data, keep))
            s.hint_frames += n

    def _end_motion(self, s):
        if s.closed:
            raise RuntimeError("Session.end_motion: the session is closed")
        s.hints_ended = True

    def _hint_rows(self, ready):
        """One row of the hint table per slot (`ops.stream_hint_table`): the staged hint frames of every hinted session go to the pinned
        staging buffer — a mask-only push as the identity template, in the form of the frames beside it — and the sessions of `ready` that
        are hinted name their window -> (rows, staged bytes)."""
        rows, lo = [None] * self.slots, 0
        host = self.hint_staged_host.numpy()
        for k, s in enumerate(self.sessions):
            if s is None or not s.motion:
                continue
            row = {}
            if s._hint_staged:
                form = next((f for f, _d, _k in s._hint_staged if f is not None), ops.STREAM_HINT_PACKED)
                w = ops.STREAM_HINT_WIDTHS[form]
                n = sum(len(keep) for _f, _d, keep in s._hint_staged)
                dst = host[lo:lo + n * w * 4].view(np.float32).reshape(n, w)
                keeps = host[lo + n * w * 4:lo + n * (w * 4 + SEED_DIMS)].reshape(n, SEED_DIMS)
                at = 0
                for _f, data, keep in s._hint_staged:
                    m = len(keep)
                    if data is not None:
                        dst[at:at + m] = data
                    elif form == ops.STREAM_HINT_PACKED:
                        dst[at:at + m] = self._ident[0].numpy()
                    else:
                        dst[at:at + m] = 0.0                                   # the zero rotation: aa_to_rot6d gives the identity's bits
                    keeps[at:at + m] = keep
                    at += m
                row.update(frames=n, src=lo, form=form, frames_before=s._hint_sent)
                lo += ops.stream_hint_chunk_bytes(n, form)
                s._hint_staged, s._hint_sent = [], s._hint_sent + n
            if s in ready:
                row.update(ready=1, window_index=s.windows, frames_before=s._hint_sent - row.get("frames", 0))
            rows[k] = row or None
        return rows, lo

    def _launch_push_hints(self):
        ops.stream_push_hints(self.hint_staged, self.hint_table, self.hint_ring_motion, self.hint_ring_keep, self.seeds, self.window_table,
                              self.window, self.status)

    # ---- the tick ---------------------------------------------------------------------------------------------------------------------------
    def _rows(self, ready):
        """One table row per slot: the staged PCM of every open session, and for the sessions of `ready` the window they run (rule 2)."""
        rows, lo = [None] * self.slots, 0
        host = self.staged_host.numpy()
        for k, s in enumerate(self.sessions):
            if s is None:
                continue
            row = {}
            if s.fmt is not None:
                lo, resample = self._resample_row(s, host, lo)
                if resample is not None:
                    row.update(resample=resample)
            elif s._staged:
                n = sum(len(c) for c in s._staged)
                np.concatenate(s._staged, out=host[lo:lo + n])
                row.update(push_count=n, push_src=lo, audio_write=(s.pushed - n) % self.ring_len)
                lo += n
                s._staged = []
            if s in ready:
                have = self.hop * (s.windows + 1)                           # codes the slot holds after this window
                valid = min(have, self.seg_len)
                upto = max(s.emitted, have - self.lag)
                row.update(ready=1, audio_read=(self.hop * SPF * s.windows) % self.ring_len, code_write=(self.hop * s.windows) % self.ring_codes,
                           seg_read=(have - valid) % self.ring_codes, seg_valid=valid, emit_row=s.emitted - (have - valid), emit_count=upto - s.emitted)
            rows[k] = row or None
        return rows, lo

    def _resample_row(self, s, host, lo):
        """The resampling batch's share of `_rows`: the session's staged frames go to the staging buffer from byte `lo` (a multiple of 16),
        its row of the second table says which outputs they complete (rule 4) -> (the next free 16-byte boundary, that row or None)."""
        k = s.slot
        nbytes = sum(len(c) for c in s._staged)
        frames = nbytes // self.frame_bytes[s.fmt]
        upto = s.pushed                                     # available(frames_in), or out_length(frames_in) once ended: all staged frames go now
        if not frames and upto == s._written:
            return lo, None
        if frames:
            np.concatenate(s._staged, out=host[lo:lo + nbytes])
            s._staged = []
        row = dict(frames=frames, src=lo, format=s.fmt, final=int(s.ended), frames_before=s._sent, outputs_before=s._written,
                   out_count=upto - s._written, hist_side=self.hist_side[k])
        if frames:
            self.hist_side[k] ^= 1                          # the launch writes the other side: the slot's next push reads that one
        s._sent, s._written = s._sent + frames, upto
        return lo + -(-nbytes // 16) * 16, row

    def _upload(self, rows, staged=0, hint_rows=None, hint_staged=0):
        if self.motion_hints:                              # the third table and the staged hint frames (rule 5)
            tab = ops.stream_hint_table(hint_rows or [None] * self.slots, hint_rows=self.hint_rows, staged_bytes=self.hint_staged.numel(),
                                        window=self.window, hop=self.hop)
            self.hint_table_host.copy_(torch.from_numpy(tab))
            if hint_staged:
                self.hint_staged[:hint_staged].copy_(self.hint_staged_host[:hint_staged], non_blocking=True)
            self.hint_table.copy_(self.hint_table_host, non_blocking=True)
            self.hint_bytes_staged = int(hint_staged)
        if self.audio_inputs is not None:                  # a resampling batch: the pushes travel in the second table, under the key "resample"
            rs_rows = [r.get("resample") if r else None for r in rows]
            rows = [{f: v for f, v in r.items() if f != "resample"} if r else None for r in rows]
            self.rs_table_host.copy_(torch.from_numpy(ops.stream_resample_table(rs_rows, formats=self.formats, ring_len=self.ring_len,
                                                                                 staged_bytes=self.staged.numel(), hist_len=self.hist_len)))
            self.rs_table.copy_(self.rs_table_host, non_blocking=True)
        tab = ops.stream_table(rows, ring_len=self.ring_len, staged_samples=self.staged.numel(), samples=self.window * SPF,
                               ring_codes=self.ring_codes, seg_len=self.seg_len, out_rows=self.hop)
        self.table_host.copy_(torch.from_numpy(tab))
        if staged:
            self.staged[:staged].copy_(self.staged_host[:staged], non_blocking=True)
        self.table.copy_(self.table_host, non_blocking=True)

    def _codes_of(self, buf):
        return {p: buf[j] for j, p in enumerate(self.parts)}

    def _launch_push(self):
        if self.audio_inputs is None:
            ops.stream_push(self.staged, self.table, self.ring, self.status)
        else:
            ops.stream_push_resample(self.staged, self.rs_table, self.formats, self.taps, self.ring, self.history, self.status)

    def _tick(self):
        """The launches of one tick: no host state, so it is capturable."""
        model, vq = self.model, self.vq
        self._launch_push()
        hints = None
        if self.motion_hints:                              # the rings, frames 0 .. 3 into the seed rows, and every slot's row of the window table
            self._launch_push_hints()
            hints = (*self._hint_store, self.window_table, self.status)
        ops.stream_windows(self.ring, self.table, self.win_audio, self.status)
        with model.collect_health():
            seed = model._window_step(vq, self.win_audio, self.speaker_id, self.tmpl_motion, self.tmpl_mask, self.seeds,
                                      self._codes_of(self.win_codes), 0, True, counter=self.nonfinite, _hints=hints)
        ops.stream_commit(self.table, self.win_codes, self.hop, self.code_ring, self.segment, seed, self.seeds, self.status)
        aa, expr, vel = vq._decode_segments(**{f"{p}_index": v for p, v in self._codes_of(self.segment).items()})
        ops.count_nonfinite_multi([aa, expr, vel], self.nonfinite)
        v = self.out_views
        ops.stream_emit(self.table, aa, expr, vel, 54, 1 / 30, self.segment, self.carry, v["poses"], v["expressions"], v["trans"], v["codes"],
                        self.status)

    def _check_flags(self, flags):
        bad, status = int(flags[0]), int(flags[1])
        if status:
            self.status.zero_()
            raise RuntimeError(f"StreamBatch: the stream kernels reported status {status} ({STATUS_TEXT})")
        if bad:
            self.nonfinite.zero_()
            raise nonfinite_error(bad, self.precision, "among the network outputs of a tick")

    def _emitted(self, views, k, n):
        codes = views["codes"][k, :n].numpy()
        return Emitted(views["poses"][k, :n].numpy().copy(), views["expressions"][k, :n].numpy().copy(), views["trans"][k, :n].numpy().copy(),
                       {p: codes[:, j].copy() for j, p in enumerate(self.parts)})

    def step(self):
        """One tick: every session that holds the samples of its next window (rule 1) runs it -> {session: Emitted}.  With no session ready
        nothing is launched and {} returned; what was pushed stays staged on the host.  A slot with two windows of backlog needs two ticks.
        Behind a FloatingPointError (non-finite logits somewhere in the batch; they are not traced to a slot) the device state of the slots
        that ran has advanced and their frames are lost: abandon the batch and build a new one."""
        ready = [s for s in self.sessions if s is not None and s.ready]
        if not ready:
            return {}
        if self._version_stamp() != self._stamp:
            raise RuntimeError("StreamBatch.step: the models' parameters changed; weights are fixed for the life of a StreamBatch — build a new one")
        rows, staged = self._rows(ready)
        self._upload(rows, staged, *(self._hint_rows(ready) if self.motion_hints else ()))
        if self.graph is not None:
            self.graph.replay()
        else:
            self._tick()
        self.ticks += 1
        self.out_host.copy_(self.out, non_blocking=True)
        if self.device.type == "cuda":
            torch.cuda.current_stream(self.device).synchronize()
        self._check_flags(self.host_views["flags"])
        out = {}
        for s in ready:
            n = int(rows[s.slot]["emit_count"])
            out[s] = self._emitted(self.host_views, s.slot, n)
            s.windows += 1
            s.emitted += n
        return out

    # ---- the end of a session ---------------------------------------------------------------------------------------------------------------
    def _close(self, s):
        """The reference's tail window (M:428-470) at its own length, the last codes decoded at their TRUE length — the right edge is
        zero-padded exactly where the reference pads it — and frames [emitted, frames_out) -> Emitted.  Frees the slot."""
        if s.closed:
            raise RuntimeError("Session.close: the session is closed")
        if s.fmt is not None:
            self._end(s)                                                    # releases the outputs held back: one more full window may be ready
        s.hints_ended = True                                                # `end_motion()`: a window that waited for hints is ready now
        if s.ready:
            raise RuntimeError("Session.close: a full window is still pending — call step() first")
        rounds, t = tail_of(s.pushed, self.pre, self.hop)
        assert s.windows == rounds, (s.windows, rounds)                     # rule 1
        result = self._finish(s, rounds, t)
        s.emitted, s.closed = self.hop * rounds + t, True
        s.hint_frames_unused = max(0, s.hint_frames - s.emitted)            # the offline set would have refused them (rule 5)
        self.sessions[s.slot] = None
        return result

    def _finish(self, s, rounds, t):
        """The device side of `close()`: the tail window of `t` frames (0: none) behind `rounds` full windows, the last decode, the emit."""
        model, vq, dev, k, pre, hop = self.model, self.vq, self.device, s.slot, self.pre, self.hop
        rows, staged = self._rows([])
        hint_rows, hint_staged = self._hint_rows([]) if self.motion_hints else (None, 0)
        push_audio = staged or any(r and "resample" in r for r in rows)    # PCM pushed since the last tick (or a filter's tail to flush)
        if push_audio or hint_staged:                                      # push-only launches
            self._upload(rows, staged, hint_rows, hint_staged)
            if push_audio:
                self._launch_push()
            if hint_staged:                                                # hints pushed since the last tick; no slot is ready: the window table is all {0, 0}
                self._launch_push_hints()
        frames_out = hop * rounds + t
        lo = max(0, hop * rounds - 2 * self.lag) if rounds else 0           # first code of the last decode: R behind the first frame to emit
        length, n_emit, n_p = frames_out - lo, frames_out - s.emitted, len(self.parts)
        result = Emitted(np.zeros((0, 165), np.float32), np.zeros((0, 100), np.float32), np.zeros((0, 3), np.float32),
                         {p: np.zeros(0, np.int64) for p in self.parts})
        if n_emit > 0:
            last = torch.zeros(n_p, 1, length, dtype=torch.int64, device=dev)
            if rounds:                                                      # codes [lo, 60 rounds) out of the ring: at most two runs per part
                segs, f = [], lo
                while f < hop * rounds:
                    n = min(hop * rounds - f, self.ring_codes - f % self.ring_codes)
                    segs += [((j * self.slots + k) * self.ring_codes + f % self.ring_codes, j * length + f - lo, n) for j in range(n_p)]
                    f += n
                table, longest = ops.segment_table(segs, self.code_ring.numel(), last.numel(), dev)
                ops.copy_segments(self.code_ring, last, table, 8, longest, self.status)
            if t:
                row = ops.stream_table([dict(ready=1, audio_read=(hop * SPF * rounds) % self.ring_len)], ring_len=self.ring_len, staged_samples=1,
                                       samples=t * SPF, ring_codes=self.ring_codes, seg_len=self.seg_len, out_rows=hop)
                audio = torch.zeros(1, t * SPF, device=dev)
                ops.stream_windows(self.ring[k:k + 1], torch.from_numpy(row).to(dev), audio, self.status)
                tail = torch.zeros(n_p, 1, t, dtype=torch.int64, device=dev)
                hints = None
                if s.motion:                                                # the tail's t rows of the slot's ring: contiguous, as every window's
                    first = k * (self.hint_rows + pre) + (hop * rounds) % self.hint_rows
                    avail = min(max(s.hint_frames - hop * rounds, 0), t)
                    hints = (*self._hint_store, torch.tensor([[first, avail]], dtype=torch.int64).to(dev), self.status)
                with model.collect_health():
                    model._window_step(vq, audio, self.speaker_id[k:k + 1], self.tmpl_motion[:1, :t], self.tmpl_mask[:1, :t], self.seeds[k:k + 1],
                                       self._codes_of(tail), 0, False, counter=self.nonfinite, _hints=hints)
                table, longest = ops.segment_table([(j * t, j * length + hop * rounds - lo, t) for j in range(n_p)], tail.numel(), last.numel(), dev)
                ops.copy_segments(tail, last, table, 8, longest, self.status)
            aa, expr, vel = vq._decode_segments(**{f"{p}_index": v for p, v in self._codes_of(last).items()})
            ops.count_nonfinite_multi([aa, expr, vel], self.nonfinite)
            out, views = self._output_buffer(1, n_emit, dev, False)
            host, host_views = self._output_buffer(1, n_emit, torch.device("cpu"), False)
            row = ops.stream_table([dict(ready=1, emit_row=s.emitted - lo, emit_count=n_emit)], ring_len=self.ring_len, staged_samples=1, samples=1,
                                   ring_codes=self.ring_codes, seg_len=length, out_rows=n_emit)
            ops.stream_emit(torch.from_numpy(row).to(dev), aa, expr, vel, 54, 1 / 30, last, self.carry[k:k + 1], views["poses"], views["expressions"],
                            views["trans"], views["codes"], self.status)
            views["flags"].copy_(self.out_views["flags"])
            host.copy_(out)
            self._check_flags(host_views["flags"])
            result = self._emitted(host_views, 0, n_emit)
        self.seeds[k].copy_(self._ident)                                   # a free slot runs on the identity seed
        if dev.type == "cuda":
            torch.cuda.current_stream(dev).synchronize()                    # the pinned staging buffers are the next tick's to refill
        return result
