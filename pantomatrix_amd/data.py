"""The training data on the device: a BEAT2 clip store resident in HBM and the loader that cuts batches out of it with one launch
(`emage_gather_clips`) and draws the random motion mask with another (`emage_motion_mask`) — the reference's
`BEAT2DatasetEamgeFootContact` + `DistributedSampler` + `DataLoader(drop_last=True)` (datasets/beat2.py:93-129, train_emage_audio.py:273-277,
310) and its `torch.rand(bs, t, 337) < mask_ratio` (train_emage_audio.py:163-165), with no host work per step.

The reference decodes a whole recording's audio and loads its whole motion file for EVERY item, to cut 64 frames out of it.  Here every
recording is loaded ONCE and uploaded (a speaker's training split is a few hundred MB), a clip is a row {first frame, first sample, recording}
of a table, and `ClipLoader.fill()` reads neither host memory nor host state: as the `prologue` of `Trainer.capture` it becomes the head of the
captured step, and a training loop's only host call per step is `trainer.replay()`.

* ``speaker_number`` / ``SpeakerMap``   BEAT2's `<speaker number>_<name>_...` recording names -> dense rows of the model's speaker tables.
* ``ClipStore``      the dataset (``from_index``: the reference's clip index JSON; ``from_arrays``: in-memory recordings);
                     ``gather_host`` is the numpy restatement of the reference's batch — the ORACLE of the GPU tests, not a fallback.
* ``epoch_order``    `DistributedSampler(shuffle=True, drop_last=False)` restated.
* ``ClipLoader``     the static batch tensors, the order buffer and the device counters."""
from __future__ import annotations

import json

import numpy as np
import torch

from . import motion_io, ops

SMPLX_FPS = 30                                          # datasets/beat2.py:106
PIECES = {"motion": "poses", "expressions": "expressions", "trans": "trans", "foot_contact": "foot_contact"}      # batch key -> recording key
NORM_MEAN, NORM_STD = 0, 1                              # beat2.py:18-19
MASK_DIMS = 337                                         # pose_dims + 3 + 4 of train_emage_audio.py:164 (55 joints x 6, trans, foot contact)
MOTION_MASK_ID = 0x6D61736B                             # Philox counter word 2 of the motion mask ("mask"): far from the dropout sites' ids


def samples_per_frame(audio_sr):
    """The reference's `int((1 / SMPLX_FPS) * self.audio_sr)` (beat2.py:112-113), quirk included: 533 at 16 kHz, not 533.33."""
    return int((1 / SMPLX_FPS) * audio_sr)


def foot_contact_path(motion_path):
    """beat2.py:104."""
    return motion_path.replace("smplxflame_30", "footcontact").replace(".npz", ".npy")


def _is_s16_mono(path, audio_sr):
    (tag, ch, sr, _, _, bits), _data = motion_io._wav_chunks(path)
    return (tag, ch, sr, bits) == (1, 1, audio_sr, 16)


def speaker_number(video_id):
    """The BEAT2 speaker number of a recording name: the leading integer before the first `_` (`2_scott_0_103_103` -> 2).  ValueError for a
    name without one."""
    head = str(video_id).split("_", 1)[0]
    if "_" not in str(video_id) or not head.isdigit():
        raise ValueError(f"speaker_number: {video_id!r} does not start with '<speaker number>_'")
    return int(head)


def _index_items(meta_paths_or_items):
    if isinstance(meta_paths_or_items, (str, dict)):
        meta_paths_or_items = [meta_paths_or_items]
    items = []
    for m in meta_paths_or_items:
        if isinstance(m, dict):
            items.append(m)
        else:
            with open(m, "r") as f:
                items.extend(json.load(f))
    return items


class SpeakerMap:
    """{BEAT2 speaker number: row of the model's speaker tables}.  `from_index` numbers the speakers of ALL items of a clip index — every
    split — densely in ascending speaker number, so a train store and a test set built from the same index agree; `len(map)` is the
    `speaker_dims` to configure.  Calling the map with an index item returns the row of its `video_id`."""

    def __init__(self, rows):
        self.rows = {int(k): int(v) for k, v in dict(rows).items()}
        if any(v < 0 for v in self.rows.values()):
            raise ValueError(f"SpeakerMap: negative rows in {self.rows}")

    @classmethod
    def from_index(cls, meta_paths_or_items):
        numbers = sorted({speaker_number(it["video_id"]) for it in _index_items(meta_paths_or_items)})
        return cls({n: i for i, n in enumerate(numbers)})

    def __len__(self):
        return max(self.rows.values()) + 1 if self.rows else 0

    def __getitem__(self, number):
        if int(number) not in self.rows:
            raise ValueError(f"SpeakerMap: speaker number {number} is not among {sorted(self.rows)}")
        return self.rows[int(number)]

    def __call__(self, item):
        return self[speaker_number(item["video_id"] if isinstance(item, dict) else item)]

    def __eq__(self, other):
        return isinstance(other, SpeakerMap) and self.rows == other.rows

    def __repr__(self):
        return f"SpeakerMap({self.rows})"


def _speaker_rows(speakers):
    """`speakers` of `ClipStore.from_index` / `recordings.RecordingSet.from_index` as a callable item -> row (None: every item is row 0)."""
    if speakers is None:
        return lambda item: 0
    if isinstance(speakers, dict):
        speakers = SpeakerMap(speakers)
    if not callable(speakers):
        raise ValueError("speakers: None, a SpeakerMap, a dict {speaker number: row} or a callable item -> row")
    return speakers


class ClipStore:
    """Every recording of a split, end to end in flat device arrays, and the clip table over them.

    recordings: dicts with `poses (F, 165)`, `expressions (F, 100)`, `trans (F, 3)`, `foot_contact (F, 4)` (cast to float32 as the reference's
    `.float()` does; the poses first go through the reference's `normalize(motion, 0, 1)` = x / (1 + 1e-7), once, at upload) and `audio`: a 1-D int16 array (mono 16-bit PCM at the model's rate, kept as it is and decoded x * 2^-15 by the kernel —
    exactly what `motion_io.load_audio` / `librosa.load` give for such a file) or float32 (numpy, or a tensor already on the device).  One format
    per store: int16 only when every recording has it.  clips: (recording index, start_idx, end_idx) triples or dicts with those keys
    (`recording`, `start_idx`, `end_idx`, optionally `video_id`).  A recording dict may carry `speaker` (int >= 0, default 0): its row of the
    model's speaker tables, kept as `speakers` ((n_recordings,) int64 on the device) and `speakers_host`.  A clip of T frames carries T * samples_per_frame samples starting at
    start_idx * samples_per_frame (beat2.py:111-114).  Refused with ValueError naming the clip: a clip that does not lie inside its recording
    in frames or in samples (the reference would collate a ragged batch), clips of unequal length, pose_fps != 30 (the reference down-samples
    `motion` only, beat2.py:106-108)."""

    def __init__(self, recordings, clips, device, audio_sr=16000, pose_fps=30):
        if pose_fps != SMPLX_FPS:
            raise ValueError(f"ClipStore: pose_fps must be {SMPLX_FPS}, not {pose_fps} (the reference down-samples `motion` only: the batch would be ragged)")
        self.device = torch.device(device)
        self.audio_sr, self.pose_fps, self.spf = int(audio_sr), int(pose_fps), samples_per_frame(audio_sr)
        if self.spf <= 0:
            raise ValueError(f"ClipStore: audio_sr {audio_sr} gives no samples per frame")
        if not recordings or not clips:
            raise ValueError("ClipStore: no recordings / no clips")
        self.recordings = [self._host_recording(i, r) for i, r in enumerate(recordings)]
        self.audio_format = "int16" if all(r["audio"].dtype == torch.int16 for r in self.recordings) else "float32"
        self.clip_list = [self._clip(i, c) for i, c in enumerate(clips)]
        self.frames = self.clip_list[0][2] - self.clip_list[0][1]
        frame0 = np.cumsum([0] + [r["frames"] for r in self.recordings])
        sample0 = np.cumsum([0] + [r["audio"].numel() for r in self.recordings])
        table = np.empty((len(self.clip_list), 3), dtype=np.int64)
        for i, (r, s, e, name) in enumerate(self.clip_list):
            rec = self.recordings[r]
            if e - s != self.frames:
                raise ValueError(f"ClipStore: clip {name} has {e - s} frames, clip {self.clip_list[0][3]} has {self.frames} (one batch shape: clips of equal length)")
            if s < 0 or e > rec["frames"]:
                raise ValueError(f"ClipStore: clip {name} = frames [{s}, {e}) does not lie inside its recording of {rec['frames']} frames")
            if e * self.spf > rec["audio"].numel():
                raise ValueError(f"ClipStore: clip {name} = samples [{s * self.spf}, {e * self.spf}) does not lie inside its recording's audio of "
                                 f"{rec['audio'].numel()} samples")
            table[i] = (frame0[r] + s, sample0[r] + s * self.spf, r)
        self.n_clips, self.total_frames, self.total_samples = len(self.clip_list), int(frame0[-1]), int(sample0[-1])
        # the flat arrays, filled recording by recording (no host-side concatenation of the whole split)
        self.arrays = {k: torch.empty(self.total_frames, ops.CLIP_WIDTHS[k], dtype=torch.float32, device=self.device) for k in PIECES}
        self.arrays["audio"] = torch.empty(self.total_samples, dtype=torch.int16 if self.audio_format == "int16" else torch.float32, device=self.device)
        for i, rec in enumerate(self.recordings):
            for k, rk in PIECES.items():
                self.arrays[k][frame0[i]:frame0[i + 1]].copy_(torch.from_numpy(rec[rk]))
            a = rec["audio"]
            self.arrays["audio"][sample0[i]:sample0[i + 1]].copy_(a if a.dtype == self.arrays["audio"].dtype else a.to(torch.float32) * (1.0 / 32768.0))
        self.clips = torch.from_numpy(table).to(self.device)
        self.speakers_host = np.asarray([r["speaker"] for r in self.recordings], dtype=np.int64)
        self.speakers = torch.from_numpy(self.speakers_host).to(self.device)
        self.has_speakers = bool(self.speakers_host.any())       # False: the reference's single speaker 0 — the loader launches what it always launched

    @staticmethod
    def _host_recording(i, r):
        out = {}
        for k, rk in PIECES.items():
            x = np.asarray(r[rk])
            if x.ndim != 2 or x.shape[1] != ops.CLIP_WIDTHS[k]:
                raise ValueError(f"ClipStore: recording {i}: {rk} has shape {x.shape}, expected (frames, {ops.CLIP_WIDTHS[k]})")
            if k == "motion":                           # beat2.py:108-109 `normalize(motion, mean=0, std=1)`, in the file's dtype: NOT the identity (std + 1e-7)
                x = (x - NORM_MEAN) / (NORM_STD + 1e-7)
            out[rk] = x.astype(np.float32, copy=False)
        out["frames"] = min(out[rk].shape[0] for rk in PIECES.values())
        for rk in PIECES.values():
            out[rk] = np.ascontiguousarray(out[rk][:out["frames"]])
        a = r["audio"]
        a = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        if a.dim() != 1 or a.dtype not in (torch.int16, torch.float32):
            raise ValueError(f"ClipStore: recording {i}: audio must be a 1-D int16 or float32 array, not {tuple(a.shape)} {a.dtype}")
        out["audio"] = a
        spk = r.get("speaker", 0)
        if isinstance(spk, bool) or not isinstance(spk, (int, np.integer)) or spk < 0:
            raise ValueError(f"ClipStore: recording {i}: speaker must be an int >= 0 (a row of the model's speaker tables), not {spk!r}")
        out["speaker"] = int(spk)
        return out

    def _clip(self, i, c):
        if isinstance(c, dict):
            r, s, e, name = c["recording"], c["start_idx"], c["end_idx"], c.get("video_id")
        else:
            (r, s, e), name = c, None
        r, s, e = int(r), int(s), int(e)
        name = f"{i} ({name})" if name is not None else str(i)
        if not 0 <= r < len(self.recordings):
            raise ValueError(f"ClipStore: clip {name} names recording {r} of {len(self.recordings)}")
        if e <= s:
            raise ValueError(f"ClipStore: clip {name} = frames [{s}, {e}) is empty")
        return r, s, e, name

    @classmethod
    def from_arrays(cls, recordings, clips, device, audio_sr=16000, pose_fps=30):
        return cls(recordings, clips, device, audio_sr=audio_sr, pose_fps=pose_fps)

    @classmethod
    def from_index(cls, meta_paths_or_items, split, device, audio_sr=16000, pose_fps=30, speakers=None):
        """The reference's clip index (beat2.py:14-17): JSON lists of dicts `video_id, motion_path, audio_path, mode, start_idx, end_idx`, given
        as one path, a list of paths, or the items themselves; filtered by `mode == split`.  Each distinct recording is loaded once:
        `motion_io.beat_format_load`, the foot-contact `.npy` next to it (beat2.py:104), and the audio — the file's int16 samples as they are
        when EVERY file is mono 16-bit PCM at `audio_sr`, else `audio.load_audio(path, audio_sr, device)` (decode, down-mix and resampling
        on the device).  speakers: where a recording's speaker-table row comes from — None: every recording is speaker 0 (the reference's
        behaviour); a `SpeakerMap`, a dict {speaker number: row} (looked up with `speaker_number(video_id)`) or a callable item -> row."""
        from . import audio as paudio
        if pose_fps != SMPLX_FPS:
            raise ValueError(f"ClipStore: pose_fps must be {SMPLX_FPS}, not {pose_fps} (the reference down-samples `motion` only: the batch would be ragged)")
        items = [it for it in _index_items(meta_paths_or_items) if it.get("mode") == split]
        if not items:
            raise ValueError(f"ClipStore.from_index: no clip with mode == {split!r}")
        keys, row_of, rows = {}, _speaker_rows(speakers), {}
        for it in items:
            k = (it["motion_path"], it["audio_path"])
            keys.setdefault(k, len(keys))
            row = int(row_of(it))
            if rows.setdefault(k, row) != row:
                raise ValueError(f"ClipStore.from_index: the clips of recording {k[0]} name different speakers ({rows[k]} and {row})")
        s16 = all(_is_s16_mono(a, audio_sr) for _m, a in keys)
        device = torch.device(device)
        recordings = []
        for motion_path, audio_path in keys:
            rec = dict(motion_io.beat_format_load(motion_path, mask=None))
            rec["foot_contact"] = np.load(foot_contact_path(motion_path))
            rec["speaker"] = rows[(motion_path, audio_path)]
            if s16:
                rec["audio"] = np.frombuffer(motion_io._wav_chunks(audio_path)[1], dtype="<i2").copy()
            elif device.type == "cuda":
                rec["audio"] = paudio.load_audio(audio_path, audio_sr, device)[0]
            else:                                       # a host store (the CPU tests): the same function without a device
                rec["audio"] = paudio.load_audio(audio_path, audio_sr)[0]
            recordings.append(rec)
        clips = [dict(recording=keys[(it["motion_path"], it["audio_path"])], start_idx=it["start_idx"], end_idx=it["end_idx"], video_id=it.get("video_id"))
                 for it in items]
        return cls(recordings, clips, device, audio_sr=audio_sr, pose_fps=pose_fps)

    def __len__(self):
        return self.n_clips

    def gather_host(self, ids, out=None):
        """The reference's batch for the clips `ids` (beat2.py:97-129 + default collation) by plain slicing of the host recordings: a dict of
        float32 CPU tensors `audio (B, T * spf)`, `motion (B, T, 165)`, `expressions`, `trans`, `foot_contact`; `out`: tensors to fill instead
        (pinned staging buffers).  The oracle of the GPU tests and the host path of tools/bench_clip_loader.py — the loader never calls it."""
        ids = [int(i) for i in ids]
        t, n = self.frames, self.frames * self.spf
        if out is None:
            out = {k: torch.empty(len(ids), t, w, dtype=torch.float32) for k, w in ops.CLIP_WIDTHS.items()}
            out["audio"] = torch.empty(len(ids), n, dtype=torch.float32)
        for b, i in enumerate(ids):
            r, s, e, _name = self.clip_list[i]
            rec = self.recordings[r]
            for k, rk in PIECES.items():
                out[k][b] = torch.from_numpy(rec[rk][s:e])
            a = rec["audio"][s * self.spf:e * self.spf]
            out["audio"][b] = a.to(torch.float32).cpu() / 32768.0 if a.dtype == torch.int16 else a.cpu()
        return out


def epoch_order(n_clips, epoch, rank=0, world=1, seed=0):
    """`torch.utils.data.distributed.DistributedSampler(range(n_clips), num_replicas=world, rank=rank, shuffle=True, seed=seed, drop_last=False)`
    after `set_epoch(epoch)`: torch.randperm from a generator seeded seed + epoch, padded to a multiple of `world` by repeating its head, then
    [rank::world] -> int64 array."""
    if n_clips <= 0 or world <= 0 or not 0 <= rank < world:
        raise ValueError(f"epoch_order: n_clips {n_clips}, rank {rank}, world {world}")
    g = torch.Generator()
    g.manual_seed(int(seed) + int(epoch))
    idx = torch.randperm(n_clips, generator=g).tolist()
    total = -(-n_clips // world) * world
    pad = total - n_clips
    idx += (idx * -(-pad // len(idx)))[:pad] if pad else []
    return np.asarray(idx[rank:total:world], dtype=np.int64)


class ClipLoader:
    """Batches of `batch` clips for one rank, cut on the device.  `batch` (dict of the five static tensors a `Trainer` takes) and `random_mask`
    ((B, T, 337) float32) live at fixed addresses; `fill()` overwrites them with the next batch of the epoch and a fresh mask:

        loader.set_epoch(0)
        trainer.capture(loader.batch, loader.random_mask, prologue=loader.fill)
        for epoch in range(epochs):
            loader.set_epoch(epoch)
            for _ in range(len(loader)):
                losses = trainer.replay()
        loader.check()

    `len(loader)`: full batches per epoch (drop_last=True, train_emage_audio.py:277).  `set_epoch` writes this rank's `epoch_order` into a fixed
    int32 device buffer and zeroes the device cursor (stream-ordered copies into fixed addresses: a captured graph sees them).  `fill()` makes two
    kernel launches and advances the two device counters (cursor, iteration) with one add; it reads no host state.  The kernel takes the batch
    position as cursor mod len(loader): a replay past the end of an epoch re-reads its first batch.  The mask ratio is a * iteration + b with
    `mask_ratio = (a, b)`, by default the reference's (iteration / 135 * 400) * 0.95 + 0.05, not clamped; `iteration` (a property over the device
    counter) counts the fills, and a resumed run sets it.

    An evaluation loader (the reference's test loader, train_emage_audio.py:276-277: `DistributedSampler(test_dataset)` at epoch 0,
    `drop_last=False`) is `ClipLoader(store, batch, drop_last=False, hold_iteration=True)`: `len()` counts the short last batch, the order
    buffer is padded to a whole batch with a valid clip id, and `valid` — one int32 on the device — holds the number of REAL clips of the
    batch `fill()` has just cut (set from the device cursor, so a captured graph carries it; `validation.Validator` hands it to
    `emage_val_metrics`).  hold_iteration: `fill()` advances the cursor but not the iteration — the reference draws the validation mask
    with the TRAINING iteration, which stands still during a validation pass; the caller sets `loader.iteration`.

    Speakers: `speaker_id` — (B, 1) int64 at a fixed address, next to `random_mask` — holds the speaker-table row of every clip of the batch
    (`Trainer.capture(..., speaker_id=loader.speaker_id)`).  A store with any non-zero speaker makes `fill()` issue one more launch
    (`emage_gather_clip_speakers`, the same cursor value as the clip gather); a store of speaker 0 only launches what it always launched and
    `speaker_id` stays zero.  speaker_dims: the model's `speaker_dims`; the store's rows are checked against it here (ValueError), since a
    captured step does not read ids back."""

    def __init__(self, store, batch, rank=0, world=1, seed=0, mask_seed=0, mask_ratio=(400 / 135 * 0.95, 0.05), drop_last=True, hold_iteration=False,
                 speaker_dims=None):
        self.store, self.batch_size, self.rank, self.world, self.seed, self.mask_seed = store, int(batch), int(rank), int(world), int(seed), int(mask_seed)
        self.mask_a, self.mask_b = float(mask_ratio[0]), float(mask_ratio[1])
        self.drop_last, self.hold_iteration = bool(drop_last), bool(hold_iteration)
        if speaker_dims is not None and int(store.speakers_host.max()) >= int(speaker_dims):
            raise ValueError(f"ClipLoader: the store holds speaker row {int(store.speakers_host.max())}; the model's speaker tables have "
                             f"{int(speaker_dims)} rows (speaker_dims)")
        per_rank = -(-store.n_clips // self.world)
        if self.batch_size <= 0:
            self.n_batches = 0
        elif self.drop_last:
            self.n_batches = per_rank // self.batch_size
        else:
            self.n_batches = -(-per_rank // self.batch_size)
        if self.n_batches <= 0:
            raise ValueError(f"ClipLoader: {store.n_clips} clips over {world} ranks give no full batch of {batch}")
        self.n_real = min(per_rank, self.n_batches * self.batch_size)         # clips of an epoch on this rank; the rest of the order buffer is padding
        dev, t = store.device, store.frames
        self.batch = {k: torch.zeros(self.batch_size, t, w, dtype=torch.float32, device=dev) for k, w in ops.CLIP_WIDTHS.items()}
        self.batch["audio"] = torch.zeros(self.batch_size, t * store.spf, dtype=torch.float32, device=dev)
        self.random_mask = torch.zeros(self.batch_size, t, MASK_DIMS, dtype=torch.float32, device=dev)
        self.speaker_id = torch.zeros(self.batch_size, 1, dtype=torch.int64, device=dev)
        self.order = torch.zeros(self.n_batches * self.batch_size, dtype=torch.int32, device=dev)
        self.counters = torch.zeros(2, dtype=torch.int32, device=dev)          # [cursor, iteration]
        self.cursor, self._iteration = self.counters[0:1], self.counters[1:2]
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.valid = torch.full((1,), self.batch_size, dtype=torch.int32, device=dev)      # real clips of the batch `fill()` cut last
        self.epoch, self.epoch_ids = None, None
        self.set_epoch(0)

    def __len__(self):
        return self.n_batches

    def set_epoch(self, epoch):
        ids = epoch_order(self.store.n_clips, epoch, self.rank, self.world, self.seed)[:self.n_batches * self.batch_size]
        if len(ids) < self.n_batches * self.batch_size:                        # drop_last=False: the short last batch is padded with a valid clip
            ids = np.concatenate([ids, np.full(self.n_batches * self.batch_size - len(ids), ids[0], dtype=ids.dtype)])
        self.epoch, self.epoch_ids = int(epoch), ids.reshape(self.n_batches, self.batch_size)
        self.order.copy_(torch.from_numpy(ids.astype(np.int32)))
        self.cursor.zero_()

    @property
    def iteration(self):
        return int(self._iteration)

    @iteration.setter
    def iteration(self, value):
        self._iteration.fill_(int(value))

    def prologue_state(self):
        """The device tensors `fill()` advances: `Trainer.capture` saves them around its warm-up step and puts them back."""
        return [self.counters] if self.drop_last else [self.counters, self.valid]

    def fill(self):
        st = self.store
        ops.gather_clips(self.order, self.cursor, self.n_batches, st.clips, st.arrays, self.batch, self.status, frames=st.frames, samples_per_frame=st.spf)
        if st.has_speakers:                                                    # the same cursor value as the gather above: it advances below
            ops.gather_clip_speakers(self.order, self.cursor, self.n_batches, st.clips, st.speakers, self.speaker_id, self.status)
        ops.motion_mask(self.random_mask, self.mask_a, self.mask_b, self.mask_seed, MOTION_MASK_ID, self._iteration)
        if not self.drop_last:                                                 # real clips of this batch, from the device cursor alone (capturable)
            pos = torch.remainder(self.cursor, self.n_batches)
            torch.clamp(self.n_real - pos * self.batch_size, max=self.batch_size, out=self.valid)
        (self.cursor if self.hold_iteration else self.counters).add_(1)

    def check(self):
        """Read the status word of the gathers so far (one device-to-host copy: call it where the losses are read anyway) and clear it."""
        bad = int(self.status)
        if bad:
            self.status.zero_()
            raise RuntimeError(f"ClipLoader: emage_gather_clips reported status {bad} (1: a clip id outside [0, {self.store.n_clips}) in the order buffer; "
                               "2: a clip table row outside the flat arrays, or — emage_gather_clip_speakers — a recording id outside the speaker "
                               "list) — those batch rows were zero-filled")
