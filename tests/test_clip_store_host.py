"""The device-resident clip store without a device: `data.ClipStore` / `epoch_order` / `ClipLoader` against the REAL reference's dataset,
sampler and loader (tests/golden/clip_store.npz, and live where the reference tree exists), the constructor's refusals, the loader's
bookkeeping over the host stand-ins of its two kernels (tests/fake_clip_ops.py), and the numpy restatement of the motion mask."""
import json
import math

import numpy as np
import pytest
import torch

import clip_store_common as cc
import fake_clip_ops
import fake_ops
from pantomatrix_amd import data, ops


@pytest.fixture(scope="module")
def fixture():
    recordings, clips = cc.make_recordings()
    return recordings, clips, data.ClipStore.from_arrays(recordings, clips, "cpu")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return cc.golden(golden_dir)


def test_fixture_has_the_edge_clips(fixture):
    _recordings, clips, store = fixture
    assert len(clips) == 13 == len(store) and store.frames == cc.CLIP and store.spf == cc.SPF == data.samples_per_frame(16000)
    assert clips[0][:2] == (0, 0) and clips[-1] == (2, cc.FRAMES[2] - cc.CLIP, cc.FRAMES[2])
    assert store.audio_format == "int16" and store.arrays["audio"].dtype == torch.int16
    assert store.total_frames == sum(cc.FRAMES) and store.total_samples == sum(f * cc.SPF + 7 for f in cc.FRAMES)


def test_from_index_equals_from_arrays(fixture, tmp_path):
    _recordings, _clips, store = fixture
    _r, _c, index = cc.make_recordings(path=str(tmp_path))
    for source in (index, [index], json.load(open(index))):
        got = data.ClipStore.from_index(source, "train", "cpu")
        assert got.n_clips == store.n_clips and got.audio_format == "int16" and got.frames == store.frames
        assert torch.equal(got.clips, store.clips)
        for k in cc.KEYS:
            assert got.arrays[k].dtype == store.arrays[k].dtype and torch.equal(got.arrays[k], store.arrays[k]), k
    held_out = data.ClipStore.from_index(index, "test", "cpu")
    assert held_out.n_clips == 1 and held_out.total_frames == cc.FRAMES[0]          # only the recording its clip names is loaded
    with pytest.raises(ValueError):
        data.ClipStore.from_index(index, "val", "cpu")


def test_other_audio_takes_the_float32_format(tmp_path):
    """One file that is not mono s16 at 16 kHz (here: stereo) turns the whole store to float32 through `load_audio`."""
    from pantomatrix_amd import motion_io
    recordings, clips, index = cc.make_recordings(path=str(tmp_path))
    stereo = np.stack([recordings[1]["audio"], recordings[1]["audio"][::-1]], axis=1)
    cc.write_wav_s16(str(tmp_path / "wave16k" / "rec1.wav"), stereo.reshape(-1), channels=2)
    store = data.ClipStore.from_index(index, "train", "cpu")
    assert store.audio_format == "float32" and store.arrays["audio"].dtype == torch.float32
    want = [motion_io.load_audio(str(tmp_path / "wave16k" / f"rec{r}.wav"), 16000)[0] for r in range(3)]
    assert torch.equal(store.arrays["audio"], torch.from_numpy(np.concatenate(want)))
    for i, (r, s, e) in enumerate(clips):
        assert torch.equal(store.gather_host([i])["audio"][0], torch.from_numpy(want[r][s * cc.SPF:e * cc.SPF])), i


def test_gather_host_equals_every_golden_batch(fixture, gold):
    _recordings, _clips, store = fixture
    assert int(gold["n_clips"]) == store.n_clips
    seen = 0
    for world, rank in cc.RANKS:
        for epoch in cc.EPOCHS:
            order, batches = cc.golden_batches(gold, world, rank, epoch)
            assert len(batches) == len(order) // cc.BATCH
            for i, want in enumerate(batches):
                cc.assert_batches_equal(store.gather_host(order[i * cc.BATCH:(i + 1) * cc.BATCH]), want, (world, rank, epoch, i))
                seen += 1
    assert seen == 24


@pytest.mark.skipif(not cc.reference_available(), reason="the reference tree is not on this machine (the golden file pins the same run)")
def test_gather_host_equals_the_live_reference(fixture, tmp_path):
    _recordings, _clips, store = fixture
    _r, _c, index = cc.make_recordings(path=str(tmp_path))
    for (world, rank, epoch), (order, batches) in cc.reference_run(index).items():
        assert np.array_equal(order, data.epoch_order(store.n_clips, epoch, rank, world))
        for i, want in enumerate(batches):
            cc.assert_batches_equal(store.gather_host(order[i * cc.BATCH:(i + 1) * cc.BATCH]), want, (world, rank, epoch, i))


def test_epoch_order_equals_the_golden_orders(gold):
    for world, rank in cc.RANKS:
        for epoch in cc.EPOCHS:
            got = data.epoch_order(int(gold["n_clips"]), epoch, rank, world)
            assert got.dtype == np.int64 and np.array_equal(got, gold[f"{cc.tag(world, rank, epoch)}_order"]), (world, rank, epoch)


@pytest.mark.parametrize("n", [1, 9, 10])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_epoch_order_equals_distributed_sampler(n, world):
    from torch.utils.data.distributed import DistributedSampler
    for seed in (0, 3):
        for rank in range(world):
            sampler = DistributedSampler(range(n), num_replicas=world, rank=rank, seed=seed)
            for epoch in (0, 1, 5):
                sampler.set_epoch(epoch)
                assert list(sampler) == data.epoch_order(n, epoch, rank, world, seed).tolist(), (n, world, rank, seed, epoch)


def test_constructor_refuses_what_the_reference_would_collate_ragged(fixture):
    recordings, clips, _store = fixture
    with pytest.raises(ValueError, match=r"clip 13 .*frames \[20, 28\).*27 frames"):                # one frame past its recording
        data.ClipStore.from_arrays(recordings, clips + [(1, 20, 28)], "cpu")
    short = [dict(r) for r in recordings]
    short[2]["audio"] = short[2]["audio"][:cc.FRAMES[2] * cc.SPF - 1]                             # one sample short of the last clip's end
    with pytest.raises(ValueError, match=r"clip 12 .*samples"):
        data.ClipStore.from_arrays(short, clips, "cpu")
    with pytest.raises(ValueError, match=r"clip 13 has 7 frames"):
        data.ClipStore.from_arrays(recordings, clips + [(0, 0, 7)], "cpu")
    with pytest.raises(ValueError, match="pose_fps"):
        data.ClipStore.from_arrays(recordings, clips, "cpu", pose_fps=15)
    named = [dict(recording=r, start_idx=s, end_idx=e, video_id=f"take{i}") for i, (r, s, e) in enumerate(clips)] + [dict(recording=0, start_idx=-1, end_idx=7, video_id="early")]
    with pytest.raises(ValueError, match=r"clip 13 \(early\)"):
        data.ClipStore.from_arrays(recordings, named, "cpu")
    exact = [dict(r) for r in recordings]
    exact[2]["audio"] = exact[2]["audio"][:cc.FRAMES[2] * cc.SPF]                                 # exactly enough: accepted
    assert data.ClipStore.from_arrays(exact, clips, "cpu").n_clips == 13


@pytest.mark.parametrize("world,rank", cc.RANKS)
def test_loader_over_the_stand_ins_reproduces_the_golden_batches(fixture, gold, world, rank):
    _recordings, _clips, store = fixture
    with fake_clip_ops.installed():
        loader = data.ClipLoader(store, cc.BATCH, rank=rank, world=world, mask_seed=5)
        assert len(loader) == len(cc.golden_batches(gold, world, rank, 0)[1]) and loader.random_mask.shape == (cc.BATCH, cc.CLIP, 337)
        addresses = {k: v.data_ptr() for k, v in loader.batch.items()}
        it = 0
        for epoch in cc.EPOCHS:
            loader.set_epoch(epoch)
            assert int(loader.cursor) == 0
            for i, want in enumerate(cc.golden_batches(gold, world, rank, epoch)[1]):
                loader.fill()
                cc.assert_batches_equal(loader.batch, want, (world, rank, epoch, i))
                a, b = loader.mask_a, loader.mask_b
                assert torch.equal(loader.random_mask.reshape(-1), torch.from_numpy(ops.motion_mask_reference(loader.random_mask.numel(), a, b, 5, data.MOTION_MASK_ID, it)))
                it += 1
                assert int(loader.cursor) == i + 1 and loader.iteration == it
        assert {k: v.data_ptr() for k, v in loader.batch.items()} == addresses
        # the cursor stands at len(loader): the next fill wraps to the epoch's first batch, and set_epoch resets it
        first = cc.golden_batches(gold, world, rank, cc.EPOCHS[-1])[1][0]
        loader.fill()
        cc.assert_batches_equal(loader.batch, first, "wrap")
        assert int(loader.cursor) == len(loader) + 1
        loader.set_epoch(0)
        assert int(loader.cursor) == 0 and loader.iteration == it + 1
        loader.fill()
        cc.assert_batches_equal(loader.batch, cc.golden_batches(gold, world, rank, 0)[1][0], "after set_epoch")
        loader.iteration = 135
        assert loader.iteration == 135
        loader.fill()
        assert float(loader.random_mask.min()) == 1.0          # ratio 400 * 0.95 + 0.05 > 1: all ones, not clamped
        loader.check()
        assert fake_ops.CALLS.count("gather_clips") == fake_ops.CALLS.count("motion_mask") == it + 3


def test_loader_reports_ids_outside_the_table(fixture):
    _recordings, _clips, store = fixture
    with fake_clip_ops.installed():
        loader = data.ClipLoader(store, 3)
        assert len(loader) == 4
        loader.order[:3] = torch.tensor([-1, 4, 13], dtype=torch.int32)
        loader.fill()
        want = store.gather_host([4])
        for k in cc.KEYS:
            assert torch.equal(loader.batch[k][1], want[k][0]) and float(loader.batch[k][0].abs().max()) == 0.0 and float(loader.batch[k][2].abs().max()) == 0.0
        with pytest.raises(RuntimeError, match="status 1"):
            loader.check()
        loader.check()                                          # cleared
    with pytest.raises(ValueError, match="no full batch"):
        data.ClipLoader(store, 14)
    with pytest.raises(ValueError, match="no full batch"):
        data.ClipLoader(store, 5, world=4)                      # ceil(13 / 4) = 4 clips per rank


# ---- the motion mask, restated ---------------------------------------------------------------------------------------------------------
def test_motion_mask_reference_shares_the_dropout_stream():
    """Same key and counter -> the same Philox words: dropout keeps u >= p, the motion mask sets u < r, so with r = p one is the complement
    of the other, element for element; another mask id or iteration is another stream."""
    n, seed, mask_id, it = 2 * 8 * 337, 0x1234567887654321, 77, 9
    for p in (0.1, 0.5):
        keep = ops.philox_dropout_reference(n, p, seed, mask_id, it) != 0
        mask = ops.motion_mask_reference(n, 0.0, p, seed, mask_id, it)
        assert mask.dtype == np.float32 and mask.shape == (n,) and set(np.unique(mask)) == {0.0, 1.0}
        assert np.array_equal(mask == 1.0, ~keep)
    base = ops.motion_mask_reference(n, 0.0, 0.5, seed, mask_id, it)
    assert not np.array_equal(base, ops.motion_mask_reference(n, 0.0, 0.5, seed, mask_id + 1, it))
    assert not np.array_equal(base, ops.motion_mask_reference(n, 0.0, 0.5, seed + 1, mask_id, it))
    assert not np.array_equal(base, ops.motion_mask_reference(n, 0.5 / (it + 1), 0.0, seed, mask_id, it + 1))
    assert np.array_equal(base, ops.motion_mask_reference(n, 0.25 / it, 0.25, seed, mask_id, it))      # the ratio is a * iteration + b
    assert np.array_equal(base[:101], ops.motion_mask_reference(101, 0.0, 0.5, seed, mask_id, it))      # a prefix: n is no multiple of 4


def test_motion_mask_reference_density_and_saturation():
    """A share of ones within 5 sigma of r for n Bernoulli(r) draws: |share - r| <= 5 sqrt(r (1 - r) / n) — derived, and checked here
    once for the seed used."""
    r, n = 0.3, 2 * 64 * 337
    share = float(ops.motion_mask_reference(n, 0.0, r, 0, data.MOTION_MASK_ID, 3).mean())
    bound = 5 * math.sqrt(r * (1 - r) / n)
    print(f"motion mask: share of ones {share:.5f} for r = {r} over {n} elements (bound {bound:.5f})")
    assert abs(share - r) <= bound
    for a, b, it in ((0.0, 1.0, 0), (0.0, 1.5, 4), (400 / 135 * 0.95, 0.05, 1)):
        assert float(ops.motion_mask_reference(4001, a, b, 1, 2, it).min()) == 1.0
    for a, b, it in ((0.0, 0.0, 0), (0.0, -0.2, 4), (-1.0, 0.5, 1)):
        assert float(ops.motion_mask_reference(4001, a, b, 1, 2, it).max()) == 0.0
