"""The clip store on the MI355X: `emage_gather_clips` against `ClipStore.gather_host` (plain slicing, the reference's batch), `emage_motion_mask`
against its numpy restatement, `ClipLoader` against the REAL reference's batches (tests/golden/clip_store.npz), argument validation, and the
loader as the prologue of a captured training step.  Order buffers and clip tables are views into larger tensors whose slack holds VALID
entries, and outputs are views inside canary frames: a missing guard shows as a wrong result, never as an access outside an allocation."""
import numpy as np
import pytest
import torch

import clip_store_common as cc
import common
from pantomatrix_amd import _lib, data, ops, training

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = -777.25
N_BATCHES = 3
_STORES = {}


def random_recordings(seed, frames, audio):
    """Full-range recordings (no golden to compress): `audio` "int16" or "float32"."""
    rng = np.random.default_rng(seed)
    out = []
    for f in frames:
        n = f * cc.SPF + 7
        out.append(dict(poses=(0.3 * rng.standard_normal((f, 165))).astype(np.float32), expressions=(0.5 * rng.standard_normal((f, 100))).astype(np.float32),
                        trans=(0.1 * rng.standard_normal((f, 3))).astype(np.float32), foot_contact=rng.integers(0, 2, (f, 4)).astype(np.float32),
                        audio=rng.integers(-32768, 32768, n).astype(np.int16) if audio == "int16" else (0.1 * rng.standard_normal(n)).astype(np.float32)))
    return out


def kernel_store(t, audio):
    """Three recordings of t + 5, t + 9 and t frames (odd audio lengths: the second and third start at odd sample offsets), clips of t frames at
    stride 3 — the first clip starts the store, the last ends it.  Built once per (t, audio)."""
    if (t, audio) not in _STORES:
        frames = (t + 5, t + 9, t)
        clips = [(r, s, s + t) for r, f in enumerate(frames) for s in range(0, f - t + 1, 3)]
        _STORES[(t, audio)] = data.ClipStore.from_arrays(random_recordings(t, frames, audio), clips, DEV)
    return _STORES[(t, audio)]


def framed(shape):
    """A canary-filled tensor one element larger on every side, and the view of `shape` inside it."""
    big = torch.full([s + 2 for s in shape], CANARY, dtype=torch.float32, device=DEV)
    return big, big[tuple(slice(1, -1) for _ in shape)]


def canaries_intact(big):
    inner = torch.zeros_like(big, dtype=torch.bool)
    inner[tuple(slice(1, -1) for _ in big.shape)] = True
    return bool((big[~inner] == CANARY).all())


def slack_view(values, pad, fill):
    """`values` as a view into a tensor with `pad` valid entries (`fill`) in front and behind."""
    values = torch.as_tensor(values)
    big = torch.empty((values.shape[0] + 2 * pad, *values.shape[1:]), dtype=values.dtype)
    big[:] = torch.as_tensor(fill, dtype=values.dtype)
    big[pad:pad + values.shape[0]] = values
    big = big.to(DEV)
    return big, big[pad:pad + values.shape[0]]


def batch_ids(store, b):
    """N_BATCHES batches of b ids: the first and the last clip of the store, ids that repeat within a batch."""
    last, mid = store.n_clips - 1, store.n_clips // 2
    rows = [[0, last, 0], [last, mid, mid], [1, 2, last]]
    return [r[:b] for r in rows]


def outputs(store, b):
    frames, outs = {}, {}
    for k, w in ops.CLIP_WIDTHS.items():
        frames[k], outs[k] = framed((b, store.frames, w))
    frames["audio"], outs["audio"] = framed((b, store.frames * store.spf))
    return frames, outs


@pytest.mark.parametrize("audio", ["int16", "float32"])
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("t", [8, 64])
def test_gather_clips_equals_gather_host(t, b, audio):
    store = kernel_store(t, audio)
    assert store.audio_format == audio and store.clip_list[0][:2] == (0, 0) and store.clip_list[-1][2] == t
    ids = batch_ids(store, b)
    _ob, order = slack_view(torch.tensor(ids, dtype=torch.int32).reshape(-1), 8, store.n_clips // 3)
    _cb, clips = slack_view(store.clips.cpu(), 2, store.clips[1].cpu())
    assert clips.is_contiguous() and clips.data_ptr() != _cb.data_ptr()
    cursor, status = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    for cur in (0, N_BATCHES - 1, N_BATCHES):                       # the first batch, the last, and the wrap back to the first
        frames, outs = outputs(store, b)
        cursor.fill_(cur)
        ops.gather_clips(order, cursor, N_BATCHES, clips, store.arrays, outs, status, frames=t, samples_per_frame=store.spf)
        want = store.gather_host(ids[cur % N_BATCHES])
        for k in cc.KEYS:
            assert torch.equal(outs[k].cpu(), want[k]), (cur, k)
            assert canaries_intact(frames[k]), (cur, k)
    assert int(status) == 0 and int(cursor) == N_BATCHES              # the kernel reads the cursor, the loader advances it


def test_ids_outside_the_table_zero_fill_and_set_the_status_word():
    store = kernel_store(8, "int16")
    _ob, order = slack_view(torch.tensor([-1, 2, store.n_clips, 0, 0, 0], dtype=torch.int32), 8, 1)
    _cb, clips = slack_view(store.clips.cpu(), 2, store.clips[1].cpu())
    cursor, status = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    frames, outs = outputs(store, 3)
    for v in outs.values():
        v.fill_(3.5)
    ops.gather_clips(order, cursor, 2, clips, store.arrays, outs, status, frames=8, samples_per_frame=store.spf)
    want = store.gather_host([2])
    for k in cc.KEYS:
        assert torch.equal(outs[k][1].cpu(), want[k][0]), k
        assert float(outs[k][0].abs().max()) == 0.0 and float(outs[k][2].abs().max()) == 0.0, k
        assert canaries_intact(frames[k]), k
    assert int(status) == 1
    cursor.fill_(1)                                                   # a clean batch leaves the (sticky) word alone
    ops.gather_clips(order, cursor, 2, clips, store.arrays, outs, status, frames=8, samples_per_frame=store.spf)
    assert int(status) == 1 and torch.equal(outs["motion"].cpu(), store.gather_host([0, 0, 0])["motion"])
    # a table row that points outside the flat arrays is refused on the device as well (status 2), without reading there
    bent = store.clips.clone()
    bent[2, 0] = store.total_frames - 7
    status.zero_()
    cursor.zero_()
    ops.gather_clips(order, cursor, 2, bent, store.arrays, outs, status, frames=8, samples_per_frame=store.spf)
    assert int(status) == 3 and float(outs["audio"][1].abs().max()) == 0.0


@pytest.mark.parametrize("n", [2 * 8 * 337, 2 * 64 * 337, 7 * 337])
def test_motion_mask_equals_its_restatement(n):
    """Bit-equal at the two batch shapes of these tests and at 7 * 337 = 2359 elements: the one length here that is NO multiple of 4 (both
    2 * 8 * 337 and 2 * 64 * 337 are), so the last Philox block is cut."""
    assert [m % 4 for m in (2 * 8 * 337, 2 * 64 * 337, 7 * 337)] == [0, 0, 3]
    a, b, seed = 400 / 135 * 0.95 / 40, 0.05, 0x0123456789ABCDEF
    it = torch.zeros(1, dtype=torch.int32, device=DEV)
    _big, out = framed((n,))
    masks = {}
    for value in (0, 7, 0):
        it.fill_(value)                                               # the kernel reads the device counter: no launch argument changes
        ops.motion_mask(out, a, b, seed, data.MOTION_MASK_ID, it)
        got = out.cpu().numpy().copy()
        assert np.array_equal(got, ops.motion_mask_reference(n, a, b, seed, data.MOTION_MASK_ID, value)), value
        assert value not in masks or np.array_equal(masks[value], got)
        masks[value] = got
    assert canaries_intact(_big) and not np.array_equal(masks[0], masks[7]) and masks[0].mean() < masks[7].mean()
    it.fill_(135)
    ops.motion_mask(out, 400 / 135 * 0.95, 0.05, seed, data.MOTION_MASK_ID, it)
    assert float(out.min()) == 1.0


@pytest.mark.parametrize("world,rank", cc.RANKS)
def test_loader_reproduces_the_golden_batches(golden_dir, world, rank):
    gold = cc.golden(golden_dir)
    if "fixture" not in _STORES:
        _STORES["fixture"] = data.ClipStore.from_arrays(*cc.make_recordings(), DEV)
    loader = data.ClipLoader(_STORES["fixture"], cc.BATCH, rank=rank, world=world)
    for epoch in cc.EPOCHS:
        loader.set_epoch(epoch)
        for i, want in enumerate(cc.golden_batches(gold, world, rank, epoch)[1]):
            loader.fill()
            cc.assert_batches_equal(loader.batch, want, (world, rank, epoch, i))
    loader.check()
    assert loader.iteration == 2 * len(loader) and int(loader.cursor) == len(loader)


def test_from_index_on_the_device(tmp_path, golden_dir):
    """The files -> `from_index` -> loader path of the README, int16 audio kept as it is."""
    _r, _c, index = cc.make_recordings(path=str(tmp_path))
    store = data.ClipStore.from_index(index, "train", DEV)
    assert store.audio_format == "int16" and store.arrays["audio"].is_cuda
    loader = data.ClipLoader(store, cc.BATCH)
    loader.fill()
    cc.assert_batches_equal(loader.batch, cc.golden_batches(cc.golden(golden_dir), 1, 0, 0)[1][0], "from_index")


def test_invalid_arguments_are_refused():
    lib = _lib.load()
    store = kernel_store(8, "int16")
    b, t = 2, 8
    order = torch.zeros(2 * b, dtype=torch.int32, device=DEV)
    cursor, status = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    outs = {k: torch.full((b, t, w), 2.0, device=DEV) for k, w in ops.CLIP_WIDTHS.items()}
    outs["audio"] = torch.full((b, t * store.spf), 2.0, device=DEV)
    A = store.arrays

    def args(**kw):
        g = lambda k, v: kw.get(k, v)
        motion = [x for k in ("motion", "expressions", "trans", "foot_contact") for x in (g("out_" + k, outs[k].data_ptr()), t * ops.CLIP_WIDTHS[k], g("row_" + k, ops.CLIP_WIDTHS[k]))]
        return [g("order", order.data_ptr()), g("n_order", order.numel()), g("cursor", cursor.data_ptr()), g("n_batches", 2), g("batch", b),
                g("clips", store.clips.data_ptr()), store.n_clips, g("frames", t), store.spf, g("poses", A["motion"].data_ptr()), A["expressions"].data_ptr(),
                A["trans"].data_ptr(), A["foot_contact"].data_ptr(), store.total_frames, g("fmt", _lib.PCM_S16), g("audio", A["audio"].data_ptr()), store.total_samples,
                g("out_audio", outs["audio"].data_ptr()), g("ld_audio", t * store.spf), *motion, g("status", status.data_ptr()), None]

    for bad in (dict(order=None), dict(cursor=None), dict(clips=None), dict(poses=None), dict(audio=None), dict(out_audio=None), dict(out_trans=None), dict(status=None),
                dict(batch=0), dict(batch=-2), dict(n_batches=0), dict(frames=0), dict(fmt=_lib.PCM_S24), dict(fmt=_lib.PCM_S32), dict(fmt=7), dict(fmt=-1),
                dict(n_order=2 * b - 1), dict(ld_audio=t * store.spf - 1), dict(row_motion=164), dict(audio=A["audio"].data_ptr() + 1)):
        assert lib.emage_gather_clips(*args(**bad)) == -1, bad
    it = torch.zeros(1, dtype=torch.int32, device=DEV)
    mask = torch.full((64,), 2.0, device=DEV)
    assert lib.emage_motion_mask(None, 64, 0.0, 0.5, 0, 0, it.data_ptr(), None) == -1
    assert lib.emage_motion_mask(mask.data_ptr(), 64, 0.0, 0.5, 0, 0, None, None) == -1
    assert lib.emage_motion_mask(mask.data_ptr(), 0, 0.0, 0.5, 0, 0, it.data_ptr(), None) == -1
    assert lib.emage_motion_mask(mask.data_ptr(), 64, float("nan"), 0.5, 0, 0, it.data_ptr(), None) == -1
    torch.cuda.synchronize()
    assert float(mask.min()) == 2.0 and all(float(v.min()) == 2.0 == float(v.max()) for v in outs.values()) and int(status) == 0       # nothing was launched
    assert lib.emage_gather_clips(*args()) == 0
    torch.cuda.synchronize()
    assert torch.equal(outs["trans"].cpu(), store.gather_host([0, 0])["trans"])


# ---- end to end: the loader feeds the training step -----------------------------------------------------------------------------------
STEP_FRAMES = (70, 90, 81)


@pytest.fixture(scope="module")
def step_store():
    recordings = random_recordings(11, STEP_FRAMES, "int16")
    for r in recordings:
        r["audio"] = (r["audio"] // 10).astype(np.int16)               # |x| < 0.1, the level of the synthetic training batches
    clips = [(r, s, s + 64) for r, f in enumerate(STEP_FRAMES) for s in range(0, f - 64 + 1, 4)]
    return data.ClipStore.from_arrays(recordings, clips, DEV)


def checksum(model):
    return float(torch.stack([v.double().sum() for v in model._flat_params().values()]).sum())


def test_step_on_a_filled_batch_equals_the_step_on_the_host_batch(step_store):
    """(a) `fill()` then `trainer.step` on the loader's tensors, against `trainer.step` on `gather_host` of the same ids with the restated mask
    uploaded: the same loss dict, bit for bit (both trainers draw their dropout masks from the same seed and step)."""
    loader = data.ClipLoader(step_store, 2, mask_seed=3)
    loader.iteration = 1                                              # ratio a + 0.05 > 1 would hide nothing but also test nothing: take a mid ratio
    loader.mask_a, loader.mask_b = 0.25, 0.05
    loader.fill()
    ids = loader.epoch_ids[0]
    model_d, vq = common.product_models(precision="fp32", device=DEV)
    model_h, _ = common.product_models(precision="fp32", device=DEV)
    got = training.Trainer(model_d, vq, seed=0).step(loader.batch, random_mask=loader.random_mask)
    host = {k: v.to(DEV) for k, v in step_store.gather_host(ids).items()}
    mask = torch.from_numpy(ops.motion_mask_reference(loader.random_mask.numel(), 0.25, 0.05, 3, data.MOTION_MASK_ID, 1)).view(loader.random_mask.shape).to(DEV)
    assert 0.2 < float(mask.mean()) < 0.4
    want = training.Trainer(model_h, vq, seed=0).step(host, random_mask=mask)
    print("step on the filled batch:", got)
    assert got == want and all(np.isfinite(v) for v in got.values())
    assert checksum(model_d) == checksum(model_h)
    loader.check()


def test_captured_step_with_the_loader_as_prologue(step_store):
    """(b) capture(..., prologue=loader.fill) + 3 replays against 3 x (fill(), replay()) of a trainer captured WITHOUT a prologue on the same
    kind of buffers: losses and a checksum of the parameters bit for bit; cursor and iteration read 3 afterwards (the warm-up step's advance
    is undone), not 4."""
    model_p, vq = common.product_models(precision="fp32", device=DEV)
    model_q, _ = common.product_models(precision="fp32", device=DEV)
    lp, lq = data.ClipLoader(step_store, 2, mask_seed=3), data.ClipLoader(step_store, 2, mask_seed=3)
    for l in (lp, lq):
        l.mask_a, l.mask_b = 0.2, 0.05
    tp = training.Trainer(model_p, vq, seed=0).capture(lp.batch, lp.random_mask, prologue=lp.fill)
    assert int(lp.cursor) == 0 and lp.iteration == 0
    lq.fill()                                                         # the plain capture's warm-up step needs a real batch in its buffers
    tq = training.Trainer(model_q, vq, seed=0).capture(lq.batch, lq.random_mask)
    lq.set_epoch(0)
    lq.iteration = 0
    seen = []
    for step in range(3):
        got = tp.replay()
        lq.fill()
        want = tq.replay()
        assert got == want, (step, got, want)
        assert checksum(model_p) == checksum(model_q), step
        assert torch.equal(lp.batch["audio"], lq.batch["audio"]) and torch.equal(lp.random_mask, lq.random_mask)
        cc.assert_batches_equal(lp.batch, step_store.gather_host(lp.epoch_ids[step]), step)
        seen.append(got["all"])
    print("captured steps fed by the loader:", seen)
    assert len(set(seen)) == 3                                        # three different batches
    assert int(lp.cursor) == 3 and lp.iteration == 3 and tp.steps_done == 3
    lp.check()
