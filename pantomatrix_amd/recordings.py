"""The test pass on the device: whole recordings of different lengths generated as ONE lock-step batch — the reference's `inference_fn`
(train_emage_audio.py:33-102, called every `test_steps` iterations) and the loop of test_emage_audio.py:96-105, which generate every
recording alone at B = 1 (`librosa.load`, `model.inference`, `motion_vq.decode(get_global_motion=True, ref_trans=trans[:, 0])`,
`beat_format_save`).  B = 1 is the worst operating point of this code: ~280 dependent launches of 64 rows per window.

No kernel learns about lengths.  The window schedule of `inference()` (M:343-470) makes the ragged batch a STATIC schedule of ordinary ones:

1. every recording runs `rounds_r = (T_r - 4) // 60` full windows of exactly 64 frames at starts 0, 60, 120, ...: window step i is an
   ordinary batch of the recordings with rounds_r > i — one shape, one start, only the row count shrinks as short recordings finish;
2. a tail window exists when remain_r > 4 and has 4 + remain_r frames (the whole recording when T_r < 64): recordings with the SAME tail
   length form one ordinary batch although their tails start at different frames;
3. the final decode is convolutional with zero padding at each recording's own end: it runs per group of recordings of EQUAL length, at
   the true length — never on a zero-padded batch.

Two data-movement kernels (csrc/recordings.hip) keep the pass free of host state, so it is capturable as one hipGraph per tuple of lengths:
`emage_gather_windows` cuts the audio windows of a step / a tail group out of the flat array of all recordings, `emage_copy_segments` gathers
a tail group's seed rows, scatters its codes into each recording's slot and packs every recording's result into one flat buffer per output
(three device-to-host copies per pass, not three per recording).  Motion hints (`masked_motion` / `mask` of `inference()`, M:343-359:
keyframes, kept body parts) are a third table-driven input: `emage_pack_motion_hints` (csrc/elementwise.hip) packs each forward's window
operand out of a per-frame hint store (`RecordingRunner(hints=True)`).

* ``window_schedule``   the schedule itself, pure Python (`windows.py`, re-exported here; the host tests restate M:364-368 / M:428-431 against it);
* ``RecordingSet``      the recordings of a split (``from_index``) or a list of waveforms / WAV files (``from_audio``) on the device;
* ``RecordingRunner``   the pass for one tuple of lengths, eager or as one captured graph;
* ``test_pass``         `inference_fn`: the index JSONs in, `<video_id>_output.npz` files and (test_list, save_list) out;
* ``generate_folder``   the same for a folder of `*.wav` files (test_emage_audio.py: no seed, zero `ref_trans`)."""
from __future__ import annotations

import glob
import json
import os

import numpy as np
import torch

from . import motion_io, ops
from ._lib import nonfinite_error
from .data import SMPLX_FPS, _is_s16_mono, _speaker_rows, foot_contact_path
from .runtime import PackedGraphs
from .windows import MODEL_SR, SEED_DIMS, SPF, Schedule, frames_of, identity_seed, window_schedule      # noqa: F401  (re-exported: `recordings.window_schedule` ...)

HINT_LD = 344                                           # row pitch of a hint store: 337 rounded up to 8 columns (32 bytes of motion, 8 of flags)
WIDTHS = (("poses", 165), ("expressions", 100), ("trans", 3))
STATUS_TEXT = ops.STATUS


def axis_angle_to_rot6d(aa):
    """`rc.axis_angle_to_rotation_6d` (T:59) in host torch arithmetic, for the few seed frames of a recording: axis-angle -> quaternion
    (small-angle branch below 1e-6) -> rotation matrix, first two rows.  (..., 3) -> (..., 6)."""
    aa = torch.as_tensor(aa, dtype=torch.float32)
    angles = torch.norm(aa, p=2, dim=-1, keepdim=True)
    half = 0.5 * angles
    small = angles.abs() < 1e-6
    safe = torch.where(small, torch.ones_like(angles), angles)
    s = torch.where(small, 0.5 - (angles * angles) / 48, torch.sin(half) / safe)
    q = torch.cat([torch.cos(half), aa * s], dim=-1)
    r, i, j, k = torch.unbind(q, -1)
    two_s = 2.0 / (q * q).sum(-1)
    return torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                        two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r)), -1)


def _hint_template(rows):
    """(rows, HINT_LD) float32: the identity template in the first 337 columns of a hint store, zero padding behind them."""
    return torch.nn.functional.pad(identity_seed(1, rows)[0], (0, HINT_LD - SEED_DIMS))


def part_columns(part):
    """The columns of the 337 (55 joints x rot6d | trans | foot contact) that belong to `part`: "upper" / "hands" / "lower" by the joint
    partition of `EmageVQModel` (M:75-90, M:103), "trans" (330:333), "contact" (333:337) -> sorted (n,) int64 array.  For building
    `mask` arrays: `mask[a:b, part_columns("upper")] = 0` keeps the upper body of frames a..b-1."""
    from .modeling_emage_audio import JOINT_MASK_HANDS, JOINT_MASK_LOWER, JOINT_MASK_UPPER
    if part == "trans":
        return np.arange(330, 333, dtype=np.int64)
    if part == "contact":
        return np.arange(333, SEED_DIMS, dtype=np.int64)
    masks = {"upper": JOINT_MASK_UPPER, "hands": JOINT_MASK_HANDS, "lower": JOINT_MASK_LOWER}
    if part not in masks:
        raise ValueError(f"part_columns: {part!r} is none of 'upper', 'hands', 'lower', 'trans', 'contact'")
    return np.array([6 * j + k for j in range(55) if masks[part][j] for k in range(6)], dtype=np.int64)


def _host_ids(ids, n, who, speaker_dims=None):
    """One speaker-table row per recording as a host (n,) int64 tensor: None -> zeros, an int -> that id for every recording."""
    if ids is None:
        ids = 0
    if isinstance(ids, (int, np.integer)) and not isinstance(ids, bool):
        ids = [int(ids)] * n
    ids = torch.as_tensor(ids).detach().cpu().reshape(-1)
    if ids.numel() != n or ids.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"{who}: speaker ids must be an int or {n} integers (one per recording), got {tuple(ids.shape)} {ids.dtype}")
    ids = ids.to(torch.int64)
    if n and (int(ids.min()) < 0 or (speaker_dims is not None and int(ids.max()) >= speaker_dims)):
        raise ValueError(f"{who}: speaker ids {ids.tolist()} outside [0, {speaker_dims if speaker_dims is not None else 'speaker_dims'})")
    return ids


def _load_wave(path, audio_sr, device, s16):
    from . import audio as paudio
    if s16:
        return np.frombuffer(motion_io._wav_chunks(path)[1], dtype="<i2").copy()
    if torch.device(device).type == "cuda":
        return paudio.load_audio(path, audio_sr, device)[0]
    return paudio.load_audio(path, audio_sr)[0]


class RecordingSet:
    """Whole recordings on the device: the flat audio array (`audio`, int16 when EVERY recording is int16 — decoded x * 2^-15 by the
    kernel — else float32) with `sample_counts` / `sample_offsets`, and per recording the motion seed `seeds` (R, 4, 337) =
    rot6d(poses[:4]) | trans[:4] | foot_contact[:4] and `ref_trans` (R, 3) = trans[0] (T:53-60, T:83).

    The poses are RAW: `inference_fn` does not apply the dataset's `normalize` that `data.ClipStore` applies.  The rest of the ground-truth
    motion is not kept unless it is a hint: with `mask=None` the forward replaces every non-seed frame by the mask embedding (M:267-268)
    and the windows re-seed themselves from their own decode (M:384-391), so only the first four frames of `masked_motion` ever reach the
    network.

    Motion hints — the model's completion use, `inference(audio, speaker_id, vq_model, masked_motion=, mask=)` (M:343-359): keyframes, a
    body part kept from a capture, a pose to hold.  masked_motion: per recording None or an (h_r, 337) float array, a PREFIX of the
    recording (h_r <= frames_r, M:352-353); mask: per recording None or an (m_r, 337) array of exactly 0 / 1 (bool or float arrays
    holding only those values are taken; anything else raises ValueError — a narrowing: the reference compares `== 0` and `== 1` and
    leaves other values to fall between), 1 = generate this element, 0 = this element is given.  As in the reference, recording r's
    motion is the identity template overwritten by its `masked_motion` prefix and its mask all ones overwritten by its `mask` prefix
    (M:348-359): `masked_motion` without `mask` influences only the seed.  Stored as `hint_motion` (F, 344) float32 / `hint_keep`
    (F, 344) uint8 on the device (columns 337.. are padding, so a group of 8 columns is 32 / 8 bytes aligned): recording r's rows
    [hint_offsets[r], hint_offsets[r] + hint_len[r]) cover max(h_r, m_r) frames, template-filled where one of the two is shorter.
    `hinted`: some recording's mask has a 0 in it — the pass then needs a runner built with `hints=True` (`RecordingRunner.for_set` does); a
    hinted set is also `seeded`, with `mask` alone too (its seed is then the identity template).
    `seeds` and `masked_motion` exclude each other: with `masked_motion`, `seeds[r]` is the first four frames of recording r's motion as
    defined above (M:379); `ref_trans` stays an argument of its own.

    speaker_ids: one row of the model's speaker tables per recording (ints >= 0), kept on the host as `speaker_ids` ((R,) int64) —
    `RecordingRunner.load` copies them into the runner's id buffers.  None (both reference loops): the set names no speakers and the
    runner keeps the ids it was built with (0 by default)."""

    def __init__(self, audios, device, seeds=None, ref_trans=None, items=None, audio_sr=MODEL_SR, seed_poses=None, speaker_ids=None,
                 masked_motion=None, mask=None):
        if seeds is not None and masked_motion is not None:
            raise ValueError("RecordingSet: pass `seeds` or `masked_motion`, not both (the seed is the first four frames of masked_motion, M:379)")
        if audio_sr != MODEL_SR:
            raise ValueError(f"RecordingSet: the model's windows are cut at {MODEL_SR} Hz (M:345), not {audio_sr}")
        if not len(audios):
            raise ValueError("RecordingSet: no recordings")
        self.device, self.audio_sr = torch.device(device), int(audio_sr)
        waves = []
        for i, a in enumerate(audios):
            a = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
            if a.dim() != 1 or a.dtype not in (torch.int16, torch.float32):
                raise ValueError(f"RecordingSet: recording {i}: audio must be a 1-D int16 or float32 array, not {tuple(a.shape)} {a.dtype}")
            waves.append(a)
        self.audio_format = "int16" if all(a.dtype == torch.int16 for a in waves) else "float32"
        dtype = torch.int16 if self.audio_format == "int16" else torch.float32
        self.sample_counts = [int(a.numel()) for a in waves]
        self.sample_offsets = np.cumsum([0] + self.sample_counts)
        self.audio = torch.empty(int(self.sample_offsets[-1]), dtype=dtype, device=self.device)
        for a, lo, hi in zip(waves, self.sample_offsets[:-1], self.sample_offsets[1:]):
            self.audio[lo:hi].copy_(a if a.dtype == dtype else a.to(torch.float32) * (1.0 / 32768.0))
        n = len(waves)
        hint_seeds = self._store_hints(masked_motion, mask)
        # a hinted set is seeded whatever it was hinted with: the seed frames are part of the hints, and with `mask` alone the seed is the
        # identity template the mask's zeros declare as given (M:348-359, M:379)
        self.seeded = seeds is not None or hint_seeds is not None or self.hinted
        if hint_seeds is not None:
            seeds = hint_seeds
        seeds = identity_seed(n) if seeds is None else torch.as_tensor(seeds, dtype=torch.float32)
        ref_trans = torch.zeros(n, 3) if ref_trans is None else torch.as_tensor(ref_trans, dtype=torch.float32)
        if tuple(seeds.shape) != (n, 4, SEED_DIMS) or tuple(ref_trans.shape) != (n, 3):
            raise ValueError(f"RecordingSet: seeds {tuple(seeds.shape)} / ref_trans {tuple(ref_trans.shape)}, expected ({n}, 4, {SEED_DIMS}) / ({n}, 3)")
        self.seeds, self.ref_trans = seeds.to(self.device).contiguous(), ref_trans.to(self.device).contiguous()
        self.speaker_ids = None if speaker_ids is None else _host_ids(speaker_ids, n, "RecordingSet")
        self.items, self.seed_poses = items, seed_poses      # seed_poses: (R, 4, 165) host tensor, the raw axis-angle frames behind `seeds` (from_index)

    def _store_hints(self, masked_motion, mask):
        """The hint store of the set (see the class docstring) -> the seeds `masked_motion` defines, (R, 4, 337), or None without it."""
        n, frames = len(self.sample_counts), self.frames
        rows = []
        for name, arg, dtype in (("masked_motion", masked_motion, np.float32), ("mask", mask, np.float32)):
            per = [None] * n if arg is None else list(arg)
            if len(per) != n:
                raise ValueError(f"RecordingSet: {name} needs one entry (an array or None) per recording, got {len(per)} for {n}")
            for r, a in enumerate(per):
                if a is None:
                    continue
                a = np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a)
                if a.ndim != 2 or a.shape[1] != SEED_DIMS or a.shape[0] > frames[r]:
                    raise ValueError(f"RecordingSet: recording {r}: {name} must be a prefix (h, {SEED_DIMS}) of its {frames[r]} frames, got {a.shape}")
                if name == "mask" and not np.isin(a, (0, 1)).all():
                    raise ValueError(f"RecordingSet: recording {r}: mask must hold exactly 0 (given) and 1 (generate)")
                per[r] = np.ascontiguousarray(a, dtype=dtype)
            rows.append(per)
        motions, masks = rows
        self.hint_len = [max(0 if a is None else a.shape[0], 0 if k is None else k.shape[0]) for a, k in zip(motions, masks)]
        self.hint_offsets = np.cumsum([0] + self.hint_len)
        self.hinted = any(k is not None and bool((k == 0).any()) for k in masks)
        total = int(self.hint_offsets[-1])
        motion = _hint_template(total).numpy()                                          # the identity template (M:348-351) ...
        keep = np.ones((total, HINT_LD), np.uint8)                                      # ... and the all-ones mask (M:356)
        for a, k, lo in zip(motions, masks, self.hint_offsets[:-1]):
            if a is not None:
                motion[lo:lo + a.shape[0], :SEED_DIMS] = a
            if k is not None:
                keep[lo:lo + k.shape[0], :SEED_DIMS] = k.astype(np.uint8)
        self.hint_motion, self.hint_keep = torch.from_numpy(motion).to(self.device), torch.from_numpy(keep).to(self.device)
        if masked_motion is None:
            return None
        seeds = identity_seed(n)
        for r, a in enumerate(motions):
            if a is not None:
                seeds[r, :min(4, a.shape[0])] = torch.from_numpy(a[:4])
        return seeds

    def __len__(self):
        return len(self.sample_counts)

    @property
    def frames(self):
        return [frames_of(n) for n in self.sample_counts]

    @classmethod
    def from_audio(cls, audios, device, seeds=None, ref_trans=None, audio_sr=MODEL_SR, speaker_ids=None, masked_motion=None, mask=None):
        """1-D waveforms (int16 / float32 arrays or tensors) or WAV paths — the test_emage_audio.py case: no motion, identity seed, zero
        `ref_trans` unless given.  Paths load by the rule of `ClipStore.from_index`.  masked_motion / mask: motion hints, one entry per
        recording (the class docstring)."""
        paths = [a for a in audios if isinstance(a, (str, os.PathLike))]
        s16 = all(_is_s16_mono(p, audio_sr) for p in paths)
        waves = [_load_wave(a, audio_sr, device, s16) if isinstance(a, (str, os.PathLike)) else a for a in audios]
        return cls(waves, device, seeds=seeds, ref_trans=ref_trans, audio_sr=audio_sr, speaker_ids=speaker_ids, masked_motion=masked_motion, mask=mask)

    @classmethod
    def from_index(cls, meta_paths, split="test", device="cuda", audio_sr=MODEL_SR, speakers=None, hint_mask=None):
        """The reference's index JSONs (one path, a list of paths, or the items), filtered by `mode == split`, then the FIRST item per
        `video_id` (T:38-42).  Each recording is loaded once: `beat_format_load`, the foot-contact `.npy` next to it, and the audio — the
        file's int16 samples when every file is mono 16-bit PCM at `audio_sr`, else `audio.load_audio` (on the device when there is one).
        speakers: as in `data.ClipStore.from_index` — None (every recording is speaker 0), a `data.SpeakerMap`, a dict {speaker number: row}
        or a callable item -> row.
        hint_mask: a callable `(item, frames) -> (frames, 337) 0 / 1 array or None` ("keep the captured upper body, generate the rest":
        `mask[:, part_columns("upper")] = 0`).  When given, every recording's WHOLE ground-truth motion — rot6d(poses) | trans |
        foot_contact, cut at the recording's `frames` — becomes its `masked_motion` and the callable's result its `mask`; the seeds are
        bit for bit those of a set built without it."""
        if isinstance(meta_paths, (str, os.PathLike)):
            meta_paths = [meta_paths]
        items = []
        for m in meta_paths:
            if isinstance(m, dict):
                items.append(m)
            else:
                with open(m, "r") as f:
                    items.extend(json.load(f))
        items = [it for it in items if it.get("mode") == split]
        seen = set()
        items = [it for it in items if not (it["video_id"] in seen or seen.add(it["video_id"]))]
        if not items:
            raise ValueError(f"RecordingSet.from_index: no item with mode == {split!r}")
        s16 = all(_is_s16_mono(it["audio_path"], audio_sr) for it in items)
        waves, seeds, ref, raw, motions, masks = [], [], [], [], [], []
        for it in items:
            rec = motion_io.beat_format_load(it["motion_path"], mask=None)
            contact = np.load(foot_contact_path(it["motion_path"]))
            poses, trans = np.asarray(rec["poses"], dtype=np.float32), np.asarray(rec["trans"], dtype=np.float32)
            if min(poses.shape[0], trans.shape[0], contact.shape[0]) < 4:
                raise ValueError(f"RecordingSet.from_index: {it['video_id']} has fewer than 4 motion frames")
            rot6d = axis_angle_to_rot6d(torch.from_numpy(poses[:4]).reshape(4, -1, 3)).reshape(4, -1)
            seeds.append(torch.cat([rot6d, torch.from_numpy(trans[:4]), torch.from_numpy(np.asarray(contact[:4], dtype=np.float32))], dim=-1))
            ref.append(torch.from_numpy(trans[0]))
            raw.append(torch.from_numpy(poses[:4].copy()))
            waves.append(_load_wave(it["audio_path"], audio_sr, device, s16))
            if hint_mask is not None:
                frames = frames_of(len(waves[-1]))
                h = min(frames, poses.shape[0], trans.shape[0], contact.shape[0])
                full = torch.cat([axis_angle_to_rot6d(torch.from_numpy(poses[:h]).reshape(h, -1, 3)).reshape(h, -1), torch.from_numpy(trans[:h]),
                                  torch.from_numpy(np.asarray(contact[:h], dtype=np.float32))], dim=-1)
                full[:4] = seeds[-1][:h]                     # the seed frames ARE today's seed, whatever a longer batch does to the last bit
                motions.append(full.numpy())
                masks.append(hint_mask(it, frames))
        row_of = _speaker_rows(speakers)
        hinted = hint_mask is not None
        return cls(waves, device, seeds=None if hinted else torch.stack(seeds), ref_trans=torch.stack(ref), items=items, audio_sr=audio_sr,
                   seed_poses=torch.stack(raw), speaker_ids=None if speakers is None else [int(row_of(it)) for it in items],
                   masked_motion=motions if hinted else None, mask=masks if hinted else None)


class _Unit:
    """One `forward` of the schedule: rows [lo, hi) of the length-sorted recordings at frame `start` (a full window), or a tail group."""
    __slots__ = ("start", "lo", "hi", "seq", "need_seed")


class _Tail:
    __slots__ = ("t", "n", "offsets", "seed_segs", "code_segs", "ranks", "ids", "hint_lo")


class _Decode:
    __slots__ = ("lo", "hi", "frames", "segs")


class RecordingRunner:
    """The test pass for recordings of `lengths_in_samples` samples each (16 kHz), in input order.

    Internally the recordings are sorted by length, longest first, so the recordings active in window step i are a PREFIX of the per-recording
    buffers (seed chain, code buffers) and recordings of equal output length are neighbours: every full-window step is one `forward` on a row
    range (split into groups of at most `max_batch` rows), reading its audio from a contiguous batch `emage_gather_windows` fills.  The
    waveform-only work (WavEncoders, audio projection, cross-attention K / V) is hoisted ahead of the sequential loop as `EmageAudioModel._windows` does,
    in chunks of at most `max_hoist_rows` (recording, window) sequences, so its memory is bounded.  Each tail group — the recordings
    with the same tail length — is one `forward`: audio and seed rows gathered, codes scattered into each recording's slot by the two kernels.
    The final decode runs per group of equal length at the true length with `get_global_motion=True` and each recording's own `ref_trans`;
    its rows are packed into one flat buffer per output, in INPUT order.  Every forward — full-window unit or tail group — is one
    `EmageAudioModel._window_step` (lean forward, codes, health flush, seed decode); non-finite outputs raise FloatingPointError.

    seeded: take the motion seeds and `ref_trans` of the `RecordingSet` handed to `__call__`; False: identity seed, zero `ref_trans`.
    speaker_id: one id for every recording (an int; both reference loops pass zeros) or one id per recording, in input order.  Ids are INPUT
    DATA like the audio: `load()` copies a set's ids into static buffers (`speaker_id`: (R, 1) in the sorted order; one small buffer per
    tail group, whose members are arbitrary recordings), and a replay with other ids of the same lengths needs no new graph.  With EQUAL ids
    (an int, or a list of equal ones) the pass issues what it always issued: one speaker / positional table of the widest unit, whose prefix
    serves every forward.  A runner built with ids that DIFFER builds the table over every recording that runs a full window and hands each
    unit its own rows, and each tail group its own ids; it serves any ids afterwards, a runner built with equal ids only equal ones
    (`load()` refuses the rest: build the runner from the set, `for_set`).  audio_dtype: the flat array's dtype (torch.float32 / int16).

    use_graph: the whole pass is ONE captured graph for this tuple of lengths; a second call with other audio of the same lengths replays
    it — the periodic test pass of a training run.  New weights reach a replay as in `validation.Validator` (`runtime.PackedGraphs`, which
    `graph` then is): the packing of the model's operand set is captured into a second graph over the same memory pool and replayed first
    whenever the model's version stamp has moved (a training step, `load_state_dict`), so the pass reads operands packed from the current
    parameters at the addresses it was captured with.  The VQ models are frozen in the reference's training (T:233-245); after changing THEM build a new runner.

    hints: False — every forward reads the read-only templates (identity pose, all-ones mask), the launch sequence of a runner without the
    argument; `load()` of a set whose `hinted` is True raises.  True — the pass honours a set's motion hints (`RecordingSet`:
    masked_motion / mask): the runner owns a hint store with a row for every frame of every recording, `hint_motion` (sum(frames_r), 344)
    float32 and `hint_keep` uint8 — 344 columns x 5 bytes per frame, ~100 MB for the 57.7 k frames (1 924 s) of the 26 recordings
    tools/bench_recordings.py measures — recording r's rows starting at its frame offset, and ONE int64 table `hint_table` with a row per (unit row) and per (tail-group member), parallel to `win_offsets` /
    `g.offsets`: {frame offset of the recording + window start, clamp(hint_len_r - start, 0, t)}.  Each forward packs its window operand
    with `ops.pack_motion_hints` from its slice of the table instead of `ops.pack_motion` from the templates; nothing else changes, the
    seed chain included.  Hints are INPUT DATA like audio and speaker ids: `load()` copies the set's hint rows into the store and rewrites
    the table's `avail` column (stream-ordered copies into fixed addresses), so a replay with other hints of any prefix lengths on the
    same recording lengths needs no new graph.  The seed frames are part of the hints: a hinted set needs a `seeded` runner (`for_set`)."""

    def __init__(self, model, vq_model, lengths_in_samples, seeded=False, use_graph=True, max_batch=64, max_hoist_rows=256, speaker_id=0,
                 audio_dtype=torch.float32, hints=False):
        dev = model.device
        model._require_device(dev)                          # an MI355X: there is no CPU path (the host tests lift this check over stand-in ops)
        on_gpu = dev.type == "cuda"
        if audio_dtype not in (torch.float32, torch.int16):
            raise ValueError("audio_dtype must be torch.float32 or torch.int16")
        c = model.config
        self.model, self.vq, self.device, self.seeded, self.hints = model, vq_model, dev, bool(seeded), bool(hints)
        self.window, self.pre = int(c.pose_length), int(c.seed_frames)
        self.max_batch, self.max_hoist_rows = int(max_batch), max(int(max_hoist_rows), int(max_batch))
        if self.max_batch <= 0 or self.pre != 4:
            raise ValueError("RecordingRunner: max_batch must be positive and the model's seed_frames 4")
        self.sample_counts = [int(n) for n in lengths_in_samples]
        self.sample_offsets = np.cumsum([0] + self.sample_counts)
        n_rec = len(self.sample_counts)
        self.schedule = sched = window_schedule([frames_of(n) for n in self.sample_counts], self.window, self.pre)
        if min(sched.frames) == 0:
            raise ValueError(f"RecordingRunner: recordings of {[t for t, f in zip(sched.lengths, sched.frames) if f == 0]} frames generate nothing "
                             "(the reference's inference() fails on them too)")
        self.order = sorted(range(n_rec), key=lambda r: -sched.lengths[r])                 # stable: input order among equal lengths
        self.rank = {r: k for k, r in enumerate(self.order)}
        self.frames_out = list(sched.frames)
        self.out_offsets = np.cumsum([0] + self.frames_out)
        self.frame_offsets = np.cumsum([0] + list(sched.lengths))                       # recording r's rows of the hint store (input order)
        self._plan(sched)
        # ---- static buffers ----
        lmax, w, mb = max(sched.lengths), self.window, min(self.max_batch, n_rec)
        self.audio = torch.zeros(int(self.sample_offsets[-1]), dtype=audio_dtype, device=dev)
        ids = _host_ids(speaker_id, n_rec, "RecordingRunner", int(c.speaker_dims))
        self.per_recording_ids = bool((ids != ids[0]).any())                           # fixed at construction: it decides the launch sequence
        self.speaker_id = torch.zeros(n_rec, 1, dtype=torch.long, device=dev)          # sorted order, as every per-recording buffer below
        self.seed0 = identity_seed(n_rec).to(dev)                                      # sorted order, as every per-recording buffer below
        self.seeds = torch.zeros(n_rec, self.pre, SEED_DIMS, device=dev)
        self.ref_trans = torch.zeros(n_rec, 1, 3, device=dev)
        self.tmpl_motion = identity_seed(mb, w).to(dev)                                # identity pose + all-ones mask (M:347-358), read-only
        self.tmpl_mask = torch.ones_like(self.tmpl_motion)
        if self.hints:                                                                 # the template's contents: a row nobody loaded is no hint
            self.hint_motion = _hint_template(int(self.frame_offsets[-1])).to(dev)
            self.hint_keep = torch.ones(self.hint_motion.shape[0], HINT_LD, dtype=torch.uint8, device=dev)
            self.hint_table = torch.tensor([[int(self.frame_offsets[r]) + s, 0] for r, s, _t in self.hint_rows], dtype=torch.int64, device=dev)
        routes = model._routes()
        self.codes = {p: torch.zeros(n_rec, lmax, dtype=torch.int64, device=dev) for p, r in routes.items() if r}
        n_win = max([c_[1] for c_ in self.chunks], default=0)
        self.win_audio = torch.zeros(max(n_win, 1), w * SPF, device=dev)
        tail_rows = max([g.n * g.t for g in self.tails], default=0)
        self.tail_audio = torch.zeros(max(tail_rows, 1) * SPF, device=dev)
        self.tail_seed = torch.zeros(mb, self.pre, SEED_DIMS, device=dev)
        self.tail_codes = {p: torch.zeros(max(tail_rows, 1), dtype=torch.int64, device=dev) for p in self.codes}
        total = int(self.out_offsets[-1])
        self.flat = tuple(torch.zeros(total, wd, device=dev) for _k, wd in WIDTHS)
        self.host = tuple(torch.zeros(total, wd, pin_memory=on_gpu) for _k, wd in WIDTHS)
        self.flags = torch.zeros(2, dtype=torch.int32, device=dev)                     # [non-finite values, status word of the two kernels]
        self.nonfinite, self.status = self.flags[0:1], self.flags[1:2]
        self.flags_host = torch.zeros(2, dtype=torch.int32, pin_memory=on_gpu)
        self._order_dev = torch.tensor(self.order, dtype=torch.long, device=dev)
        self.set_speaker_ids(ids)
        self.precision = model.precision
        self.graph = None
        self._pass()                                                                    # packs weights, warms the allocator, validates shapes
        if on_gpu:
            torch.cuda.synchronize(dev)
        if use_graph and on_gpu:
            self.graph = PackedGraphs(model, vq_model, self._pass, "RecordingRunner: the pass")

    # ---- the static plan (host, once) ----------------------------------------------------------------------------------------------
    def _plan(self, sched):
        dev, w, hop = self.model.device, self.window, self.window - self.pre
        srt_rounds = [sched.rounds[r] for r in self.order]
        has_tail = [sched.remain[r] > self.pre for r in self.order]
        units, offsets = [], []
        self.hint_rows = []                             # (recording, window start, frames) per row of `hint_table`: the units' rows, then the tail groups'
        for i in range(max(srt_rounds, default=0)):
            active = sum(1 for r in srt_rounds if r > i)                                # a prefix: rounds is monotone in the length
            for lo in range(0, active, self.max_batch):
                u = _Unit()
                u.start, u.lo, u.hi, u.seq = i * hop, lo, min(lo + self.max_batch, active), len(offsets)
                u.need_seed = any(srt_rounds[k] > i + 1 or has_tail[k] for k in range(u.lo, u.hi))
                offsets += [int(self.sample_offsets[self.order[k]]) + u.start * SPF for k in range(u.lo, u.hi)]
                self.hint_rows += [(self.order[k], u.start, w) for k in range(u.lo, u.hi)]
                units.append(u)
        # hoisting chunks: whole units, at most max_hoist_rows sequences each -> (first sequence, sequences, units)
        self.chunks = []
        for u in units:
            n = u.hi - u.lo
            if self.chunks and self.chunks[-1][1] + n <= self.max_hoist_rows:
                s0, cnt, us = self.chunks[-1]
                self.chunks[-1] = (s0, cnt + n, us + [u])
            else:
                self.chunks.append((u.seq, n, [u]))
        self.units = units
        self.win_offsets = torch.tensor(offsets, dtype=torch.int64, device=dev) if offsets else None
        lmax, n_rec = max(sched.lengths), len(self.order)
        self.tails = []
        for t in sorted(sched.tails, reverse=True):
            members = sched.tails[t]
            for lo in range(0, len(members), self.max_batch):
                grp = members[lo:lo + self.max_batch]
                g = _Tail()
                g.t, g.n = t, len(grp)
                g.offsets = torch.tensor([int(self.sample_offsets[r]) + s * SPF for r, s in grp], dtype=torch.int64, device=dev)
                g.seed_segs = ops.segment_table([(self.rank[r], j, 1) for j, (r, _s) in enumerate(grp)], n_rec, g.n, dev)[0]
                g.code_segs = ops.segment_table([(j * t, self.rank[r] * lmax + s, t) for j, (r, s) in enumerate(grp)], g.n * t, n_rec * lmax, dev)[0]
                g.ranks = torch.tensor([self.rank[r] for r, _s in grp], dtype=torch.long, device=dev)
                g.ids = torch.zeros(g.n, 1, dtype=torch.long, device=dev)               # the members' speaker ids (`set_speaker_ids`)
                g.hint_lo = len(self.hint_rows)
                self.hint_rows += [(r, s, t) for r, s in grp]
                self.tails.append(g)
        self.decodes = []
        k = 0
        while k < n_rec:
            f = sched.frames[self.order[k]]
            hi = k + 1
            while hi < n_rec and hi - k < self.max_batch and sched.frames[self.order[hi]] == f:
                hi += 1
            d = _Decode()
            d.lo, d.hi, d.frames = k, hi, f
            d.segs = ops.segment_table([(j * f, int(self.out_offsets[self.order[k + j]]), f) for j in range(hi - k)], (hi - k) * f,
                                       int(self.out_offsets[-1]), dev)[0]
            self.decodes.append(d)
            k = hi

    @property
    def steps(self):
        """`forward` calls of one pass (full-window units + tail groups)."""
        return len(self.units) + len(self.tails)

    @property
    def mean_batch(self):
        """Mean rows per `forward` of the pass."""
        rows = sum(u.hi - u.lo for u in self.units) + sum(g.n for g in self.tails)
        return rows / max(self.steps, 1)

    # ---- the pass: launches only, no host state ---------------------------------------------------------------------------------------
    def _sliced_tables(self, tables, lo, n):
        """Rows of the speaker / positional tables for the recordings [lo, lo + n) the tables were built over."""
        from .modeling_emage_audio import _X
        m0, m1 = lo * self.window, (lo + n) * self.window
        f0 = tables["face0"]
        face0 = _X(f0.a[m0:m1], f0.a[m0:m1] if f0.r is f0.a else f0.r[m0:m1], f0.h2r, f0.ln)
        return dict(spk_body=tables["spk_body"][m0:m1], face0=face0, pos_spk=tables["pos_spk"][m0:m1], t=self.window)

    def set_speaker_ids(self, ids):
        """One speaker-table row per recording (input order; an int: the same for all) into the static id buffers — stream-ordered copies
        into fixed addresses, so a captured pass reads them at its next replay.  Checked on the host against the model's `speaker_dims`."""
        ids = _host_ids(ids, len(self.order), "RecordingRunner", int(self.model.config.speaker_dims))
        if not self.per_recording_ids and bool((ids != ids[0]).any()):
            raise ValueError("RecordingRunner: this runner was built with equal speaker ids (its pass shares one speaker table); build one with "
                             "the ids that differ (RecordingRunner(..., speaker_id=[...]) / for_set) to run per-recording ids")
        self.speaker_id.copy_(ids[self.order].reshape(-1, 1), non_blocking=True)
        if self.per_recording_ids:
            for g in self.tails:
                g.ids.copy_(self.speaker_id.index_select(0, g.ranks))

    def _hints_of(self, row0, n):
        """The `_hints` argument of a unit / tail group whose table rows are [row0, row0 + n): None without hints."""
        if not self.hints:
            return None
        return self.hint_motion[:, :SEED_DIMS], self.hint_keep[:, :SEED_DIMS], self.hint_table[row0:row0 + n], self.status

    def set_hints(self, recording_set):
        """A set's hint rows into the store and the `avail` column of the table: stream-ordered copies into fixed addresses.  Rows of the
        store behind a recording's `hint_len` keep what an earlier set left there; no table row reaches them."""
        rs = recording_set
        for r, (n, lo) in enumerate(zip(rs.hint_len, rs.hint_offsets[:-1])):
            if n > self.schedule.lengths[r]:
                raise ValueError(f"RecordingRunner: recording {r} carries {n} hinted frames, more than its {self.schedule.lengths[r]} frames")
            if n:
                fo = int(self.frame_offsets[r])
                self.hint_motion[fo:fo + n].copy_(rs.hint_motion[lo:lo + n], non_blocking=True)
                self.hint_keep[fo:fo + n].copy_(rs.hint_keep[lo:lo + n], non_blocking=True)
        avail = [min(max(int(rs.hint_len[r]) - s, 0), t) for r, s, t in self.hint_rows]
        self.hint_table[:, 1].copy_(torch.tensor(avail, dtype=torch.int64))

    def _pass(self):
        """The three phases in order; the tool times them one by one."""
        self._full_windows()
        self._tail_groups()
        self._decode()

    def _full_windows(self):
        from .modeling_emage_audio import _Ctx, Fork
        model, vq, w = self.model, self.vq, self.window
        self.nonfinite.zero_()
        self.seeds.copy_(self.seed0)
        with model.collect_health():
            tables = None
            if self.units:
                # equal ids: the table of the widest unit, a prefix of it for every unit; ids that differ: the table of every recording that
                # runs a full window (a prefix of the sorted order), each unit reads the rows of its own recordings
                nmax = max(u.hi for u in self.units) if self.per_recording_ids else max(u.hi - u.lo for u in self.units)
                tables = model._speaker_tables(_Ctx(model._engine()), self.speaker_id[:nmax], nmax, w)
            for s0, cnt, units in self.chunks:
                win = self.win_audio[:cnt]
                ops.gather_windows(self.audio, self.win_offsets[s0:s0 + cnt], win, self.status)
                feats = None
                if model.hoist_audio:                       # the waveform-only work of the chunk's windows: one set of launches on `cnt` sequences
                    with Fork(self.device, 3, model.concurrent) as fk:
                        feats = model._audio_features(_Ctx(model._engine()), win, cnt, w, True, fk, 1, 2)
                    if feats["ta"] != w:
                        feats = None
                for u in units:
                    n, k0 = u.hi - u.lo, u.seq - s0
                    f = None
                    if feats is not None:
                        f = model._feats_of_clips(feats, k0, n, w)
                    row0 = u.lo if self.per_recording_ids else 0
                    seed = model._window_step(vq, win[k0:k0 + n], self.speaker_id[row0:row0 + n], self.tmpl_motion[:n], self.tmpl_mask[:n],
                                              self.seeds[u.lo:u.hi], {p: v[u.lo:u.hi] for p, v in self.codes.items()}, u.start, u.need_seed,
                                              counter=self.nonfinite, _audio_feats=f, _tables=self._sliced_tables(tables, row0, n),
                                              _hints=self._hints_of(u.seq, n))
                    if seed is not None:
                        self.seeds[u.lo:u.hi].copy_(seed)
                del feats

    def _tail_groups(self):
        model, vq, pre = self.model, self.vq, self.pre
        with model.collect_health():
            for g in self.tails:
                n, t = g.n, g.t
                a = self.tail_audio[:n * t * SPF].view(n, t * SPF)
                ops.gather_windows(self.audio, g.offsets, a, self.status)
                ops.copy_segments(self.seeds, self.tail_seed, g.seed_segs, pre * SEED_DIMS * 4, 1, self.status)
                model._window_step(vq, a, g.ids if self.per_recording_ids else self.speaker_id[:n], self.tmpl_motion[:n, :t], self.tmpl_mask[:n, :t],
                                   self.tail_seed[:n], {p: v[:n * t].view(n, t) for p, v in self.tail_codes.items()}, 0, False,
                                   counter=self.nonfinite, _hints=self._hints_of(g.hint_lo, n))
                for p, v in self.tail_codes.items():
                    ops.copy_segments(v, self.codes[p], g.code_segs, 8, t, self.status)

    def _decode(self):
        vq = self.vq
        for d in self.decodes:
            sel = {f"{p}_index": v[d.lo:d.hi, :d.frames] for p, v in self.codes.items()}
            pred = vq.decode(**sel, get_global_motion=True, ref_trans=self.ref_trans[d.lo:d.hi])
            outs = [pred["motion_axis_angle"].contiguous(), pred["expression"].contiguous(), pred["trans"].contiguous()]
            ops.count_nonfinite_multi(outs, self.nonfinite)
            for src, dst, (_k, wd) in zip(outs, self.flat, WIDTHS):
                ops.copy_segments(src, dst, d.segs, wd * 4, d.frames, self.status)

    # ---- one pass end to end ------------------------------------------------------------------------------------------------------------
    def load(self, recording_set):
        """Copy a set's audio and speaker ids (and, when `seeded`, its seeds and `ref_trans`; with `hints`, its motion hints) into the runner's
        input buffers (stream-ordered)."""
        rs = recording_set
        if rs.hinted and not (self.hints and self.seeded):
            raise ValueError("RecordingRunner: the set carries motion hints (a mask with a 0 in it); build the runner with hints=True and "
                             "seeded=True (RecordingRunner.for_set does both)")
        if list(rs.sample_counts) != self.sample_counts:
            raise ValueError("RecordingRunner: this runner was built for other recording lengths (one runner, one graph, per tuple of lengths)")
        if rs.audio.dtype != self.audio.dtype:
            raise ValueError(f"RecordingRunner: the set's audio is {rs.audio.dtype}, the runner was built with audio_dtype={self.audio.dtype}")
        self.audio.copy_(rs.audio, non_blocking=True)
        if rs.speaker_ids is not None:
            self.set_speaker_ids(rs.speaker_ids)
        if self.seeded:
            self.seed0.copy_(rs.seeds.to(self.device).index_select(0, self._order_dev))
            self.ref_trans.copy_(rs.ref_trans.to(self.device).index_select(0, self._order_dev).view(-1, 1, 3))
        if self.hints:
            self.set_hints(rs)

    def run_device(self):
        """One pass over the current input buffers, on the current stream; the results stay in `flat` (rows in input order)."""
        if self.graph is None:
            self._pass()
        else:
            self.graph.replay()                             # packs first when the model's version stamp has moved

    def __call__(self, recording_set=None):
        """-> [(poses (T_r, 165), expressions (T_r, 100), trans (T_r, 3))] per recording in input order: numpy views of pinned buffers,
        valid until the next call."""
        if recording_set is not None:
            self.load(recording_set)
        self.run_device()
        for h, d in zip(self.host, self.flat):
            h.copy_(d, non_blocking=True)
        self.flags_host.copy_(self.flags, non_blocking=True)
        if self.device.type == "cuda":
            torch.cuda.current_stream(self.device).synchronize()
        bad, status = int(self.flags_host[0]), int(self.flags_host[1])
        if status:
            self.status.zero_()
            raise RuntimeError(f"RecordingRunner: the data-movement kernels reported status {status} ({STATUS_TEXT})")
        if bad:
            raise nonfinite_error(bad, self.precision, "among the network outputs / the generated motion")
        host = [h.numpy() for h in self.host]
        return [tuple(h[self.out_offsets[r]:self.out_offsets[r + 1]] for h in host) for r in range(len(self.sample_counts))]

    def codes_of(self, r):
        """The code indices of recording `r` (input order) from the last pass: {part: (frames,) int64 device tensor}."""
        return {p: v[self.rank[r], :self.frames_out[r]] for p, v in self.codes.items()}

    @classmethod
    def for_set(cls, model, vq_model, recording_set, **kw):
        kw.setdefault("seeded", recording_set.seeded)
        kw.setdefault("hints", recording_set.hinted)
        if recording_set.speaker_ids is not None:
            kw.setdefault("speaker_id", recording_set.speaker_ids)
        return cls(model, vq_model, recording_set.sample_counts, audio_dtype=recording_set.audio.dtype, **kw)


def _save_outputs(results, names, audio_paths, save_path, pose_fps):
    os.makedirs(save_path, exist_ok=True)
    save_list = []
    for (poses, expressions, trans), name, audio_path in zip(results, names, audio_paths):
        out = os.path.join(save_path, f"{name}_output.npz")
        motion_io.beat_format_save(out, poses, upsample=SMPLX_FPS // pose_fps, expressions=expressions, trans=trans)      # T:91
        save_list.append({"audio_path": audio_path, "motion_path": out, "video_id": name})
    return save_list


def test_pass(model, vq, meta_paths, save_path, runner=None, pose_fps=None, device=None, speakers=None, hint_mask=None):
    """`inference_fn` (T:33-102): generate every test recording of the index JSONs and write `<video_id>_output.npz`
    -> (test_list, save_list) with the reference's keys.  runner: a `RecordingRunner` built for these recordings (the periodic test pass of
    a training run keeps one and replays its graph) or any callable `recording_set -> [(poses, expressions, trans)]`; None builds one.
    speakers: where each recording's speaker-table row comes from (`RecordingSet.from_index`; None: speaker 0, as the reference).
    hint_mask: `(item, frames) -> 0 / 1 mask or None` — complete each recording's ground-truth motion where the mask is 1 and keep it where
    it is 0 (`RecordingSet.from_index`); a `runner` handed in must then have been built with hints=True."""
    if device is None:
        device = getattr(runner, "device", None) or model.device
    rs = RecordingSet.from_index(meta_paths, "test", device, speakers=speakers, hint_mask=hint_mask)
    if runner is None:
        runner = RecordingRunner.for_set(model, vq, rs)
    if pose_fps is None:
        pose_fps = int(getattr(getattr(model, "config", None), "pose_fps", SMPLX_FPS))
    results = runner(rs)
    save_list = _save_outputs(results, [it["video_id"] for it in rs.items], [it["audio_path"] for it in rs.items], save_path, pose_fps)
    return rs.items, save_list


test_pass.__test__ = False                               # a library function, not a pytest case


def generate_folder(model, vq, audio_folder, save_folder, runner=None, pose_fps=None, speaker_id=0, masked_motion=None, mask=None):
    """test_emage_audio.py:96-105: every `*.wav` of `audio_folder` (sorted) -> `<stem>_output.npz` in `save_folder`, no seed and zero
    `ref_trans` -> save_list.  speaker_id: the speaker-table row of every file (an int) or a callable `path -> row`; 0 (the default, what
    the reference passes) names no speakers: a `runner` handed in keeps the ids it was built with.  masked_motion / mask: motion hints, one
    entry (an array or None) per file in sorted order (`RecordingSet`)."""
    paths = sorted(glob.glob(os.path.join(audio_folder, "*.wav")))
    if not paths:
        raise ValueError(f"generate_folder: no *.wav in {audio_folder}")
    ids = [int(speaker_id(p)) for p in paths] if callable(speaker_id) else (int(speaker_id) or None)
    rs = RecordingSet.from_audio(paths, getattr(runner, "device", None) or model.device, speaker_ids=ids, masked_motion=masked_motion, mask=mask)
    if runner is None:
        runner = RecordingRunner.for_set(model, vq, rs)
    if pose_fps is None:
        pose_fps = int(getattr(getattr(model, "config", None), "pose_fps", SMPLX_FPS))
    names = [os.path.splitext(os.path.basename(p))[0] for p in paths]
    return _save_outputs(runner(rs), names, paths, save_folder, pose_fps)
