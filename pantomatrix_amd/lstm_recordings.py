"""DisCo / CaMN on whole recordings of different lengths as ONE batch — the loops of the reference's test_disco_audio.py and
test_camn_audio.py, which push every WAV file of a folder whole through the model at B = 1 and write `<name>_output.npz` with
`upsample = 30 // pose_fps`.  For these models B = 1 is the worst shape: a step of the recurrence costs the same dependent chain whether
1 or 256 clips ride along, so N recordings one by one cost sum(T_i) steps per LSTM layer and one batch costs max(T_i).

Only the recurrence learns about lengths (`emage_lstm_layer_lengths`, csrc/lstmseq.hip; `_LstmAudioModel.forward_ragged`): padding the
audio would move the WavEncoder's zero padding and the backward direction's start away from each recording's own end.

* ``plan_batches``          sort by length, cut into batches under `max_batch` and the kernels' two size limits — pure Python;
* ``LstmRecordingRunner``   the pass for one tuple of lengths, eager or captured as one hipGraph;
* ``generate_folder_lstm``  a folder of `*.wav` in, `<stem>_output.npz` files out."""
from __future__ import annotations

import glob
import os

import numpy as np
import torch

from . import motion_io, ops
from ._lib import EmageKernelError, nonfinite_error
from .data import SMPLX_FPS
from .modeling_lstm_audio import ragged_batch_limit
from .recordings import RecordingSet, _host_ids


def plan_batches(frames, hidden, max_batch=256):
    """frames: output frames t_b per recording (input order) -> (order, batches): `order` the recording ids sorted by length, longest
    first (ties in input order), `batches` consecutive runs of `order`.  A batch holds at most `max_batch` recordings and stays inside
    `ragged_batch_limit` at its own longest recording; similar lengths meet in a batch, so its padding stays small.  ValueError: no
    recordings, or a single recording that is past the limits on its own."""
    frames = [int(t) for t in frames]
    if not frames:
        raise ValueError("plan_batches: no recordings")
    if int(max_batch) < 1:
        raise ValueError(f"plan_batches: max_batch {max_batch} must be at least 1")
    order = sorted(range(len(frames)), key=lambda i: -frames[i])
    batches = []
    for i in order:
        if batches and len(batches[-1]) < max_batch and ragged_batch_limit(len(batches[-1]) + 1, frames[batches[-1][0]], hidden) is None:
            batches[-1].append(i)
            continue
        why = ragged_batch_limit(1, frames[i], hidden)
        if why:
            raise ValueError(f"plan_batches: recording {i}: {why}")
        batches.append([i])
    return order, batches


def padded_share(frames, batches):
    """1 - sum(t_b) / sum over batches of B * Tmax: the share of the padded rows the row-wise stages and the recurrence carry for nothing."""
    rows = sum(len(ids) * max(frames[i] for i in ids) for ids in batches)
    return 1.0 - sum(frames) / rows


class LstmRecordingRunner:
    """The ragged pass of a DisCo / CaMN model for ONE tuple of recording lengths: the recordings sorted by length and cut into batches
    (`plan_batches`), every batch one `forward_ragged` (per-recording WavEncoders, the padded row-wise stages, one persistent
    `emage_lstm_layer_lengths` launch per LSTM layer), the non-finite count over the padded outputs and the recurrences' lost-block
    words folded into one counter — captured as ONE hipGraph (`use_graph`).  `runner(recording_set)` -> [(motion (t_b, pose_dims),
    axis_angle (t_b, 165))] in input order: numpy views of pinned buffers, valid until the next call.  A non-finite result or a lost
    block raises on every call.

    New weights (`load_state_dict`, an optimiser step ...) are seen by the next call: the model's version stamp is compared on every call
    and the graph is captured afresh when it moved.  (Packing the LSTM weights regroups the gate rows through host index tables, which a
    graph cannot capture — so the pass is re-captured on the new operand set instead of re-packing inside a second graph.)"""

    def __init__(self, model, sample_counts, use_graph=True, max_batch=256, speaker_id=0, audio_dtype=torch.float32, seed_frames=4):
        dev = model.device
        if dev.type != "cuda":
            raise RuntimeError("LstmRecordingRunner needs the model on an MI355X device")
        if audio_dtype not in (torch.float32, torch.int16):
            raise ValueError(f"LstmRecordingRunner: audio_dtype {audio_dtype} (float32 or int16)")
        self.model, self.device, self.seed_frames = model, dev, int(seed_frames)
        self.sample_counts = [int(n) for n in sample_counts]
        self.frames = model.ragged_frames(self.sample_counts)
        self.order, self.batches = plan_batches(self.frames, model.config.hidden_size, max_batch)
        self.padded_share = padded_share(self.frames, self.batches)
        n = len(self.sample_counts)
        self.sample_offsets = np.cumsum([0] + self.sample_counts)
        self.audio = torch.zeros(int(self.sample_offsets[-1]), dtype=audio_dtype, device=dev)
        self._audio_f32 = self.audio if audio_dtype == torch.float32 else torch.zeros(self.audio.shape, dtype=torch.float32, device=dev)
        self.speaker_ids = torch.zeros(n, dtype=torch.long, device=dev)          # in the runner's (sorted) order: a batch reads a slice
        self.set_speaker_ids(speaker_id)
        self.nonfinite = torch.zeros(2, dtype=torch.int32, device=dev)           # [non-finite results, lost blocks of the recurrences]
        self.nonfinite_host = torch.zeros(2, dtype=torch.int32, pin_memory=True)
        self.out_offsets = np.cumsum([0] + self.frames)
        total = int(self.out_offsets[-1])
        self.host = (torch.empty(total, model.config.pose_dims, dtype=torch.float32, pin_memory=True),
                     torch.empty(total, 165, dtype=torch.float32, pin_memory=True))
        self.use_graph, self.graph, self._stamp, self.out = bool(use_graph), None, None, None
        if self.use_graph:
            self._capture()

    @classmethod
    def for_set(cls, model, recording_set, use_graph=True, max_batch=256, **kw):
        if recording_set.speaker_ids is not None:
            kw.setdefault("speaker_id", recording_set.speaker_ids)
        return cls(model, recording_set.sample_counts, use_graph=use_graph, max_batch=max_batch, audio_dtype=recording_set.audio.dtype, **kw)

    def set_speaker_ids(self, ids):
        """One speaker-table row per recording (input order), or an int for all."""
        ids = _host_ids(ids, len(self.sample_counts), "LstmRecordingRunner", getattr(self.model.config, "speaker_dims", None))
        self.speaker_ids.copy_(ids[self.order].to(self.device), non_blocking=False)

    def _pass(self):
        """One pass over the input buffers on the current stream -> per recording (input order) the (motion, axis_angle) device views."""
        if self._audio_f32 is not self.audio:                                    # int16 samples: x * 2^-15, what a float WAV decoder returns
            self._audio_f32.copy_(self.audio)
            self._audio_f32.mul_(1.0 / 32768.0)
        self.nonfinite.zero_()
        out, lo = [None] * len(self.sample_counts), 0
        for ids in self.batches:
            waves = [self._audio_f32[self.sample_offsets[i]:self.sample_offsets[i + 1]] for i in ids]
            results, buffers = self.model._forward_ragged(waves, self.speaker_ids[lo:lo + len(ids)], self.seed_frames)
            lo += len(ids)
            for group in buffers:                    # the padded rows are computed from zeros: the count covers the whole buffers
                for t in group:
                    ops.count_nonfinite(t.contiguous(), self.nonfinite[:1])
            # batches of equal size share the recurrences' scratch: fold this batch's lost-block words before the next one re-zeroes them
            self.model.fold_kernel_health(self.nonfinite[1:], batch=len(ids))
            for i, r in zip(ids, results):
                out[i] = (r["motion"].reshape(self.frames[i], -1), r["motion_axis_angle"])
        return out

    def _capture(self):
        self.graph = None
        self.out = self._pass()                      # warm-up: packs the operands, builds the constant tables and the recurrences' scratch
        torch.cuda.synchronize(self.device)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            self.out = self._pass()
        # what the captured launches read: alive as long as the graph is
        self.graph, self._stamp, self._operands = graph, self.model._version_stamp(), (self.model._packed, dict(self.model._templates))

    def load(self, recording_set):
        """Copy a set's audio (and speaker ids, when it names any) into the runner's input buffers (stream-ordered)."""
        rs = recording_set
        if list(rs.sample_counts) != self.sample_counts:
            raise ValueError("LstmRecordingRunner: this runner was built for other recording lengths (one runner, one graph, per tuple of lengths)")
        if rs.audio.dtype != self.audio.dtype:
            raise ValueError(f"LstmRecordingRunner: the set's audio is {rs.audio.dtype}, the runner was built with audio_dtype={self.audio.dtype}")
        self.audio.copy_(rs.audio, non_blocking=True)
        if rs.speaker_ids is not None:
            self.set_speaker_ids(rs.speaker_ids)

    def run_device(self):
        """One pass over the current input buffers, on the current stream; the results stay in `out` (input order)."""
        if not self.use_graph:
            self.out = self._pass()
            return
        if self.model._version_stamp() != self._stamp:
            self._capture()                          # new weights: a new operand set, a new graph
        self.graph.replay()

    def __call__(self, recording_set=None):
        if recording_set is not None:
            self.load(recording_set)
        self.run_device()
        for r, pair in enumerate(self.out):
            for h, d in zip(self.host, pair):
                h[self.out_offsets[r]:self.out_offsets[r + 1]].copy_(d, non_blocking=True)
        self.nonfinite_host.copy_(self.nonfinite, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        if int(self.nonfinite_host[0]):
            raise nonfinite_error(self.nonfinite_host[0], self.model.precision, "in the generated motion")
        if int(self.nonfinite_host[1]):
            raise EmageKernelError("emage_lstm_layer: a block timed out waiting for its group (blocks not co-resident: another kernel holding CUs?); "
                                   "the motion of this pass is invalid")
        host = [h.numpy() for h in self.host]
        return [tuple(h[self.out_offsets[r]:self.out_offsets[r + 1]] for h in host) for r in range(len(self.sample_counts))]


def generate_folder_lstm(model, audio_folder, save_folder, runner=None, speaker_id=0):
    """test_disco_audio.py / test_camn_audio.py: every `*.wav` of `audio_folder` (sorted) in ONE ragged pass -> `<stem>_output.npz` in
    `save_folder` (`beat_format_save(..., upsample=30 // pose_fps)`; the root translation is written as zeros — the reference derives its
    default from the licensed SMPL-X body model, which `motion_io` does not carry) -> {output file name: the model's frame count t_b,
    what the scripts' `inference` returns}.  speaker_id: the speaker-table row of every file (an int) or a callable
    `path -> row`.  runner: an `LstmRecordingRunner` built for these files' lengths (it keeps its graph between calls); None builds one."""
    paths = sorted(glob.glob(os.path.join(audio_folder, "*.wav")))
    if not paths:
        raise ValueError(f"generate_folder_lstm: no *.wav in {audio_folder}")
    ids = [int(speaker_id(p)) for p in paths] if callable(speaker_id) else [int(speaker_id)] * len(paths)
    rs = RecordingSet.from_audio(paths, getattr(runner, "device", None) or model.device, speaker_ids=ids)
    if runner is None:
        runner = LstmRecordingRunner.for_set(model, rs, seed_frames=int(getattr(model.config, "seed_frames", 4)))
    upsample = SMPLX_FPS // int(model.config.pose_fps)
    os.makedirs(save_folder, exist_ok=True)
    written = {}
    for (_motion, axis_angle), path in zip(runner(rs), paths):
        stem = os.path.splitext(os.path.basename(path))[0]
        out = os.path.join(save_folder, f"{stem}_output.npz")
        motion_io.beat_format_save(out, axis_angle, trans=np.zeros((axis_angle.shape[0], 3), dtype=axis_angle.dtype), upsample=upsample)
        written[os.path.basename(out)] = int(axis_angle.shape[0])
    return written
