"""Generate tests/golden/clip_store.npz from the REAL reference (build container only):
    python tests/golden/make_golden_clip_store.py
The fixture of tests/clip_store_common.py (three recordings, 13 training clips of 8 frames) is written as the files the reference's dataset
reads; its `BEAT2DatasetEamgeFootContact`, torch's `DistributedSampler` and `DataLoader(batch_size=2, drop_last=True, num_workers=0)` then run
over them, and for epochs 0 and 1 at (world, rank) in {(1, 0), (2, 0), (2, 1)} the sampler's order and every collated batch are recorded — arrays
only.  The audio is stored as int16: the reference's float32 samples are x * 2^-15 of the file's 16-bit values, which is checked here."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import clip_store_common as cc  # noqa: E402


def main():
    assert cc.reference_available(), "needs the reference tree"
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        _recordings, clips, index = cc.make_recordings(path=tmp)
        runs = cc.reference_run(index)
    out["n_clips"] = np.int64(len(clips))
    for (world, rank, epoch), (order, batches) in runs.items():
        t = cc.tag(world, rank, epoch)
        out[f"{t}_order"] = order
        assert batches and all(set(b) == set(cc.KEYS) for b in batches)
        for k in cc.KEYS:
            a = np.stack([b[k].numpy() for b in batches])
            assert a.dtype == np.float32
            if k == "audio":
                q = a * np.float32(32768.0)
                assert np.array_equal(q, np.round(q)) and np.abs(q).max() <= 32768
                a = q.astype(np.int16)
                assert np.array_equal(a.astype(np.float32) / np.float32(32768.0), np.stack([b[k].numpy() for b in batches]))
            out[f"{t}_{k}"] = a
        print(t, "order", order.tolist(), "batches", len(batches), {k: tuple(batches[0][k].shape) for k in cc.KEYS})
    path = os.path.join(HERE, "clip_store.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
