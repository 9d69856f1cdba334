"""Shared pieces of the clip-store tests: the three-recording fixture (in memory and as the files the reference's dataset reads), the run of
the REAL reference over those files (tests/golden/make_golden_clip_store.py records it; the live test repeats it where the reference tree
exists), and accessors of tests/golden/clip_store.npz."""
import importlib.util
import json
import os
import struct
import sys
import types

import numpy as np
import torch

from oracle import reference_harness as rh
from pantomatrix_amd import motion_io

SEED = 7
FRAMES = (19, 27, 11)
CLIP, STRIDE, SPF = 8, 3, 533
BATCH = 2
EPOCHS = (0, 1)
RANKS = ((1, 0), (2, 0), (2, 1))                  # (world, rank)
# the fixture draws from few values (16 audio levels with both ends of the s16 range, motion in quarters): a misplaced offset still shows in
# every row, and the recorded batches compress to a fraction of full-entropy noise
AUDIO_LEVELS = np.array([-32768, -20001, -12345, -4097, -513, -255, -2, -1, 0, 1, 3, 254, 1023, 8191, 16385, 32767], dtype=np.int16)
KEYS = ("audio", "motion", "expressions", "trans", "foot_contact")


def make_recordings(seed=SEED, frames=FRAMES, clip=CLIP, stride=STRIDE, path=None):
    """-> (recordings, clips): float32 poses / expressions / trans (multiples of 1/4), {0, 1} foot contact and mono s16 audio of frames * 533 + 7 samples per
    recording; clips of `clip` frames at stride `stride` as (recording, start, end) — the first starts at frame 0 of a recording, the last ends
    at the last frame of the last one.  With `path`: also written as .npz / .npy / .wav files plus `index.json` there (one extra clip with
    mode "test", which a train split must not see) -> (recordings, clips, index path)."""
    rng = np.random.default_rng(seed)
    recordings, clips = [], []
    for r, f in enumerate(frames):
        q = lambda w: (rng.integers(-8, 8, (f, w)) / 4.0).astype(np.float32)
        recordings.append(dict(poses=q(165), expressions=q(100), trans=q(3), foot_contact=rng.integers(0, 2, (f, 4)).astype(np.float32),
                               audio=AUDIO_LEVELS[rng.integers(0, len(AUDIO_LEVELS), f * SPF + 7)]))
        clips += [(r, s, s + clip) for s in range(0, f - clip + 1, stride)]
    assert clips[0][1] == 0 and clips[-1][0] == len(frames) - 1 and clips[-1][2] == frames[-1]
    if path is None:
        return recordings, clips
    return recordings, clips, write_files(path, recordings, clips)


def write_wav_s16(path, samples, rate=16000, channels=1):
    data = np.asarray(samples, dtype="<i2").tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 1, channels, rate, rate * 2 * channels, 2 * channels, 16)
                + b"data" + struct.pack("<I", len(data)) + data)


def write_files(path, recordings, clips):
    for d in ("smplxflame_30", "footcontact", "wave16k"):
        os.makedirs(os.path.join(path, d), exist_ok=True)
    items = []
    paths = []
    for r, rec in enumerate(recordings):
        m, a = os.path.join(path, "smplxflame_30", f"rec{r}.npz"), os.path.join(path, "wave16k", f"rec{r}.wav")
        motion_io.beat_format_save(m, rec["poses"], expressions=rec["expressions"], trans=rec["trans"])
        np.save(os.path.join(path, "footcontact", f"rec{r}.npy"), rec["foot_contact"])
        write_wav_s16(a, rec["audio"])
        paths.append((m, a))
    for i, (r, s, e) in enumerate(clips):
        items.append(dict(video_id=f"rec{r}_{i}", motion_path=paths[r][0], audio_path=paths[r][1], mode="train", start_idx=s, end_idx=e))
    items.insert(2, dict(video_id="held_out", motion_path=paths[0][0], audio_path=paths[0][1], mode="test", start_idx=1, end_idx=1 + (clips[0][2] - clips[0][1])))
    index = os.path.join(path, "index.json")
    with open(index, "w") as f:
        json.dump(items, f)
    return index


def reference_available():
    return rh.available() and os.path.isfile(os.path.join(rh.REFERENCE_ROOT, "datasets", "beat2.py"))


def reference_run(index, batch=BATCH, epochs=EPOCHS, ranks=RANKS):
    """The real reference over the written files: `BEAT2DatasetEamgeFootContact`, `DistributedSampler` and `DataLoader(batch_size, drop_last=True,
    num_workers=0)` -> {(world, rank, epoch): (the sampler's order, [batch dicts])}.  Its datasets/beat2.py is loaded by file path (an installed
    `datasets` package shadows the directory name); `smplx` is stubbed, and a stub `librosa.load` delegates to `motion_io.load_audio`, which is
    exact for 16 kHz mono s16 input."""
    from torch.utils.data import DataLoader
    from torch.utils.data.distributed import DistributedSampler
    librosa = types.ModuleType("librosa")
    librosa.load = lambda path, sr=22050: motion_io.load_audio(path, sr)
    saved = {k: sys.modules.get(k) for k in ("smplx", "librosa")}
    sys.modules.setdefault("smplx", types.ModuleType("smplx"))
    sys.modules["librosa"] = librosa
    try:
        spec = importlib.util.spec_from_file_location("reference_beat2", os.path.join(rh.REFERENCE_ROOT, "datasets", "beat2.py"))
        beat2 = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(beat2)
        cfg = types.SimpleNamespace(data=types.SimpleNamespace(meta_paths=[index]), model=types.SimpleNamespace(joint_mask=None, pose_fps=30, audio_sr=16000))
        ds = beat2.BEAT2DatasetEamgeFootContact(cfg, "train")
        out = {}
        for world, rank in ranks:
            sampler = DistributedSampler(ds, num_replicas=world, rank=rank)
            loader = DataLoader(ds, batch_size=batch, sampler=sampler, drop_last=True, num_workers=0)
            for epoch in epochs:
                sampler.set_epoch(epoch)
                out[(world, rank, epoch)] = (np.asarray(list(iter(sampler)), dtype=np.int64), [dict(b) for b in loader])
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return out


def tag(world, rank, epoch):
    return f"w{world}r{rank}e{epoch}"


def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "clip_store.npz"))


def golden_batches(g, world, rank, epoch):
    """-> (order, [batch dicts of float32 CPU tensors]) as tests/golden/make_golden_clip_store.py stored them: per key one stacked
    (n_batches, B, ...) array; the audio as the int16 values x of the reference's float32 x * 2^-15."""
    t = tag(world, rank, epoch)
    n = g[f"{t}_motion"].shape[0]
    batches = []
    for i in range(n):
        b = {k: torch.from_numpy(g[f"{t}_{k}"][i].astype(np.float32)) for k in KEYS if k != "audio"}
        b["audio"] = torch.from_numpy(g[f"{t}_audio"][i].astype(np.float32) / np.float32(32768.0))
        batches.append(b)
    return g[f"{t}_order"], batches


def assert_batches_equal(got, want, what=""):
    assert set(got) == set(want) == set(KEYS), (what, sorted(got), sorted(want))
    for k in KEYS:
        a, b = got[k].cpu(), want[k].cpu()
        assert a.dtype == b.dtype == torch.float32 and a.shape == b.shape and torch.equal(a, b), (what, k, a.shape, b.shape)
