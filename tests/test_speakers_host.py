"""Per-clip speaker ids without a GPU: the oracle step restated with ids (tools/workloads.py) against the golden of the REAL reference step
with four speakers (tests/golden/train_step_speakers.npz), `data.speaker_number` / `SpeakerMap`, the loader's `speaker_id` buffer over the
host twins of its kernels (tests/fake_speaker_ops.py), and the ids `RecordingRunner` hands to each forward over stand-in ops."""
import os

import numpy as np
import pytest
import torch

import fake_ops
import fake_speaker_ops
import speaker_common as sc
from pantomatrix_amd import data, ops, recordings as R


# ---- 1. the helper the GPU tests rely on -------------------------------------------------------------------------------------------------
def test_oracle_step_with_ids_matches_the_reference_golden(golden_dir):
    """The bars of tests/test_train_oracle.py::test_train_step_matches_golden, plus every ROW of the two speaker tables' gradients and their
    values after Adam (whole-tensor norms cannot see two rows swapped)."""
    g = sc.golden(golden_dir)
    assert int(g["speaker_dims"]) == 4 and g["speaker_ids"].tolist() == [2, 0, 2, 1]
    r = sc.oracle_step(g, backward=True)
    loss, grads, new_sd = r["losses"], r["grads"], r["new_sd"]
    for k in sc.LOSS_KEYS:
        assert abs(loss[k] - float(g["loss_" + k])) <= 2e-4 * max(1.0, abs(float(g["loss_" + k]))), k
    names = [str(n) for n in g["grad_names"]]
    assert sorted(names) == sorted(grads)
    gmax = max(float(v.abs().max()) for v in grads.values())
    for n, norm, first, shadowed, s in zip(names, g["grad_norms"], g["grad_first"], g["shadowed"], g["param_sum_after"]):
        if shadowed:
            assert float(grads[n].abs().max()) < 1e-4 * gmax, n
            continue
        assert abs(float(grads[n].norm()) - float(norm)) <= 5e-3 * float(norm) + 1e-6 * gmax, n
        assert abs(float(grads[n].reshape(-1)[0]) - float(first)) <= 5e-3 * float(grads[n].abs().max()) + 1e-6 * gmax, n
        assert abs(float(new_sd[n].double().sum()) - float(s)) <= 3e-5 * new_sd[n].numel() ** 0.5 + 2e-3, n
    for n in sc.TABLES:
        want, after = torch.from_numpy(g["grad/" + n]), torch.from_numpy(g["after/" + n])
        assert want.shape == (4, 768) and float(want[3].abs().max()) == 0.0 and float(want[2].norm()) > float(want[0].norm()) > 0
        for row in range(4):
            assert abs(float(grads[n][row].norm()) - float(want[row].norm())) <= 5e-3 * float(want[row].norm()), (n, row)
            assert float((grads[n][row] - want[row]).norm()) <= 5e-3 * float(want[row].norm()), (n, row)
        assert float(grads[n][3].abs().max()) == 0.0 and torch.equal(new_sd[n][3], after[3])
        assert float((new_sd[n] - after).abs().max()) <= 3e-5, n


def test_oracle_step_without_ids_is_unchanged():
    """speaker_id=None returns exactly what the helper returned before it took ids: the oracle's own `train_step_losses`."""
    from oracle import emage_train_oracle as tro
    from tools import workloads
    a = workloads.oracle_train_step_recorded(11, 0, bs=2)
    b = workloads.oracle_train_step_recorded(11, 0, bs=2, speaker_id=[0, 0])
    assert a["losses"] == b["losses"] and torch.equal(a["random_mask"], b["random_mask"])
    assert tro.train_step_losses.__module__ == "oracle.emage_train_oracle"          # the restated step is put back


# ---- 2. speaker numbers and maps -------------------------------------------------------------------------------------------------------
def test_speaker_number_and_speaker_map():
    assert data.speaker_number("2_scott_0_103_103") == 2 and data.speaker_number("25_goto_1_1_1") == 25
    for bad in ("scott_0_1_1", "", "2", "_2_scott", "2a_scott_0"):
        with pytest.raises(ValueError):
            data.speaker_number(bad)
    items = [dict(video_id="4_lawrence_0_1_1", mode="train"), dict(video_id="2_scott_0_3_3", mode="test"), dict(video_id="1_wayne_0_2_2", mode="val"),
             dict(video_id="2_scott_0_5_5", mode="train")]
    smap = data.SpeakerMap.from_index(items)                       # every split, dense, ascending speaker number
    assert smap.rows == {1: 0, 2: 1, 4: 2} and len(smap) == 3
    assert [smap(it) for it in items] == [2, 1, 0, 1] and smap[4] == 2
    assert smap == data.SpeakerMap.from_index(list(reversed(items)))
    with pytest.raises(ValueError):
        smap[3]
    with pytest.raises(ValueError):
        data.SpeakerMap({1: -1})
    explicit = data._speaker_rows({2: 5, 4: 0})                    # an explicit dict {speaker number: row}
    assert explicit(items[0]) == 0 and explicit(items[1]) == 5 and len(data.SpeakerMap({2: 5, 4: 0})) == 6
    with pytest.raises(ValueError):
        explicit(items[2])
    assert data._speaker_rows(None)(items[0]) == 0 and data._speaker_rows(lambda it: 7)(items[0]) == 7


def test_from_index_takes_speakers_from_the_map(tmp_path):
    """Recordings rec0 / rec1 / rec2 of the written split renamed to BEAT2 names of speakers 4, 2 and 4: the map numbers them over ALL
    splits (the held-out test clip included), the train store and the test set agree, and a recording whose clips name two speakers is
    refused."""
    import json

    import clip_store_common as cc
    _recordings, clips, index = cc.make_recordings(path=str(tmp_path))
    items = json.load(open(index))
    number = {"rec0": 4, "rec1": 2, "rec2": 4}
    for it in items:
        rec = os.path.splitext(os.path.basename(it["motion_path"]))[0]
        it["video_id"] = f"{number[rec]}_{rec}_{it['video_id']}"
    smap = data.SpeakerMap.from_index(items)
    assert smap.rows == {2: 0, 4: 1}
    store = data.ClipStore.from_index(items, "train", "cpu", speakers=smap)
    assert store.speakers_host.tolist() == [1, 0, 1] and store.speakers.dtype == torch.int64 and store.has_speakers
    assert data.ClipStore.from_index(items, "train", "cpu", speakers={2: 3, 4: 0}).speakers_host.tolist() == [0, 3, 0]
    assert data.ClipStore.from_index(items, "train", "cpu", speakers=lambda it: 5).speakers_host.tolist() == [5, 5, 5]
    plain = data.ClipStore.from_index(items, "train", "cpu")
    assert plain.speakers_host.tolist() == [0, 0, 0] and not plain.has_speakers
    rs = R.RecordingSet.from_index(items, "test", "cpu", speakers=smap)
    assert rs.speaker_ids.tolist() == [1] and R.RecordingSet.from_index(items, "test", "cpu").speaker_ids is None
    items[1]["video_id"] = "2_" + items[1]["video_id"]
    with pytest.raises(ValueError, match="different speakers"):
        data.ClipStore.from_index(items, "train", "cpu", speakers=data.SpeakerMap.from_index(items))


def test_store_and_loader_validate_rows():
    with fake_speaker_ops.installed():
        store = sc.speaker_store("cpu")
        assert store.speakers_host.tolist() == [2, 0, 2] and store.has_speakers and store.speakers.dtype == torch.int64
        assert not sc.speaker_store("cpu", speakers=(None, None, 0)).has_speakers
        for bad in (-1, 1.5, True):
            with pytest.raises(ValueError):
                sc.speaker_store("cpu", speakers=(0, bad, 0))
        data.ClipLoader(store, 2, speaker_dims=3)
        with pytest.raises(ValueError, match="speaker_dims"):
            data.ClipLoader(store, 2, speaker_dims=2)


# ---- 3. the loader's ids on the host twin --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drop_last", [True, False])
@pytest.mark.parametrize("world", [1, 2])
def test_loader_speaker_ids_follow_the_epoch_order(world, drop_last):
    with fake_speaker_ops.installed():
        store = sc.speaker_store("cpu")
        for rank in range(world):
            loader = data.ClipLoader(store, 2, rank=rank, world=world, drop_last=drop_last, hold_iteration=not drop_last)
            addr = loader.speaker_id.data_ptr()
            assert tuple(loader.speaker_id.shape) == (2, 1) and loader.speaker_id.dtype == torch.int64
            for epoch in (0, 1):
                loader.set_epoch(epoch)
                ids = data.epoch_order(store.n_clips, epoch, rank, world, 0)
                if len(ids) % 2 and not drop_last:
                    ids = np.concatenate([ids, ids[:1]])             # the short last batch repeats a valid clip; its id is that clip's
                n_batches = len(ids) // 2
                assert len(loader) == n_batches
                for k in range(n_batches + 1):                       # one past the end: the cursor wraps to the first batch
                    fake_ops.CALLS.clear()
                    loader.fill()
                    assert fake_ops.CALLS.count("gather_clip_speakers") == 1 and fake_ops.CALLS.count("gather_clips") == 1
                    clips = ids[(k % n_batches) * 2:(k % n_batches) * 2 + 2]
                    want = [int(store.speakers_host[store.clip_list[int(c)][0]]) for c in clips]
                    assert loader.speaker_id.reshape(-1).tolist() == want, (world, rank, epoch, k)
                    assert loader.speaker_id.data_ptr() == addr
            loader.check()
            seen = set()
            loader.set_epoch(0)
            for _ in range(len(loader)):
                loader.fill()
                seen.update(loader.speaker_id.reshape(-1).tolist())
            assert seen == {0, 2}


def test_store_without_speakers_issues_no_extra_call():
    with fake_speaker_ops.installed():
        store = sc.speaker_store("cpu", speakers=(None, 0, None))
        loader = data.ClipLoader(store, 2, speaker_dims=1)
        fake_ops.CALLS.clear()
        for _ in range(4):
            loader.fill()
        assert [c for c in fake_ops.CALLS if c in ("gather_clips", "motion_mask", "gather_clip_speakers")] == ["gather_clips", "motion_mask"] * 4
        assert not loader.speaker_id.any()


def test_speaker_gather_twin_reports_bad_rows():
    with fake_speaker_ops.installed():
        store = sc.speaker_store("cpu")
        loader = data.ClipLoader(store, 2)
        loader.order[0] = 99
        loader.fill()
        assert loader.speaker_id[0, 0] == 0
        with pytest.raises(RuntimeError, match="status"):
            loader.check()


def test_embedding_backward_twin_states_the_kernel_contract():
    g = torch.randn(5 * 3, 7, generator=torch.Generator().manual_seed(0))
    got = fake_speaker_ops.embedding_backward(g, torch.tensor([3, 0, 9, -1, 3]), 4)
    per_clip = g.reshape(5, 3, 7).sum(1)
    assert torch.allclose(got[3], per_clip[0] + per_clip[2] + per_clip[4], atol=1e-6) and torch.allclose(got[0], per_clip[1] + per_clip[3], atol=1e-6)
    assert not got[1].any() and not got[2].any()


def test_argument_checks_of_the_new_entry_points_run_without_a_gpu():
    from pantomatrix_amd import _lib
    lib = _lib.load()
    ok = dict(g=8, ldg=4, ids=8, B=2, T=3, D=4, S=2, dw=8, lddw=4, ws=8, ws_bytes=64)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.emage_embedding_backward(a["g"], a["ldg"], a["ids"], a["B"], a["T"], a["D"], a["S"], a["dw"], a["lddw"], a["ws"], a["ws_bytes"], None)
    for bad in (dict(g=None), dict(ids=None), dict(dw=None), dict(ws=None), dict(B=0), dict(T=0), dict(D=0), dict(D=4097, ldg=5000, lddw=5000, ws_bytes=1 << 20),
                dict(S=0), dict(S=1025), dict(ldg=3), dict(lddw=3), dict(ws_bytes=63), dict(ws=12)):
        assert call(**bad) == -1, bad
    assert lib.emage_embedding_backward_workspace_bytes(2, 4) == 64 and lib.emage_embedding_backward_workspace_bytes(0, 4) == 0
    assert lib.emage_gather_clip_speakers(None, 4, 8, 2, 2, 8, 1, 8, 1, 8, 8, None) == -1
    assert lib.emage_gather_clip_speakers(8, 3, 8, 2, 2, 8, 1, 8, 1, 8, 8, None) == -1          # the order buffer is shorter than n_batches * batch
    assert lib.emage_gather_clip_speakers(8, 4, 8, 2, 2, 8, 1, 8, 0, 8, 8, None) == -1
    assert lib.emage_gather_clip_speakers(8, 4, 8, 2, 2, 8, 1, 12, 1, 8, 8, None) == -1         # 8-byte words at their natural alignment


def test_eager_ids_are_validated_on_the_host():
    from pantomatrix_amd import training
    with pytest.raises(ValueError, match="speaker_dims"):
        training.speaker_ids(torch.tensor([0, 4]), 2, "cpu", 4)
    with pytest.raises(ValueError):
        training.speaker_ids(torch.tensor([0, -1]), 2, "cpu", 4)
    with pytest.raises(ValueError):
        training.speaker_ids(torch.tensor([0, 1, 2]), 2, "cpu", 4)
    with pytest.raises(ValueError):
        training.speaker_ids(torch.tensor([0.0, 1.0]), 2, "cpu", 4)
    assert training.speaker_ids(None, 3, "cpu", 1).tolist() == [[0], [0], [0]]
    ids = torch.tensor([3, 1])
    assert training.speaker_ids(ids, 2, "cpu", 4).data_ptr() == ids.data_ptr()                  # used in place: a graph reads the caller's buffer


# ---- 4. the recording runner hands every forward the ids of ITS recordings ---------------------------------------------------------------
RUNNER_FRAMES = (70, 130, 70, 64, 40)
RUNNER_IDS = (2, 0, 1, 0, 2)


def test_runner_forwards_receive_the_ids_of_their_recordings():
    """Five recordings, max_batch = 2: sorted by length [1, 0, 2, 3, 4]; window step 0 splits into rows [0, 2) and [2, 4) (lo > 0), the
    10-frame tail group holds recordings 0 and 1 (ids 2 and 0) and a second group recording 2.  Every forward's `speaker_id` argument and
    the rows of the speaker table it is handed are those of its recordings; a runner with equal ids shares one table as before."""
    import fake_recording_ops
    from pantomatrix_amd import synthetic
    model, vq = sc.product_models(3)
    waves = [synthetic.synthetic_audio(1, synthetic.samples_for_frames(f), seed=77 + k)[0] for k, f in enumerate(RUNNER_FRAMES)]
    seen = []
    real = model.forward

    def spy(audio, speaker_id, *a, **kw):
        tab = kw.get("_tables")
        seen.append((speaker_id.reshape(-1).tolist(), audio.shape[0], None if tab is None else tab["spk_body"][::tab["t"], :4].clone()))
        return real(audio, speaker_id, *a, **kw)

    with fake_recording_ops.installed(), torch.no_grad():
        rs = R.RecordingSet.from_audio(waves, "cpu", speaker_ids=RUNNER_IDS)
        runner = R.RecordingRunner.for_set(model, vq, rs, use_graph=False, max_batch=2)
        assert runner.per_recording_ids and runner.order == [1, 0, 2, 3, 4]
        assert [(u.start, u.lo, u.hi) for u in runner.units] == [(0, 0, 2), (0, 2, 4), (60, 0, 1)]
        assert [(g.t, g.n) for g in runner.tails] == [(40, 1), (10, 2), (10, 1)]
        model.forward = spy
        try:
            runner(rs)
            first = list(seen)
            del seen[:]
            other = (1, 1, 0, 2, 0)
            runner(R.RecordingSet.from_audio(waves, "cpu", speaker_ids=other))
            second = list(seen)
            del seen[:]
            same = R.RecordingRunner(model, vq, rs.sample_counts, use_graph=False, max_batch=2, speaker_id=[1] * 5)
            equal = list(seen)                                       # the pass its constructor runs
        finally:
            del model.forward
        with pytest.raises(ValueError, match="equal speaker ids"):
            same.load(rs)
        with pytest.raises(ValueError):
            R.RecordingRunner(model, vq, rs.sample_counts, use_graph=False, speaker_id=[0, 1, 2, 3, 0])      # speaker_dims = 3
    table = model.speaker_embedding_body.weight.detach()
    members = [[1, 0], [2, 3], [1], [4], [0, 1], [2]]                # units (sorted order), then the tail groups (40 frames; 10 frames twice, in input order)
    for ids_in, run in ((RUNNER_IDS, first), (other, second)):
        assert len(run) == len(members)
        for (got, n, rows), recs in zip(run, members):
            want = [ids_in[r] for r in recs]
            assert got == want and n == len(recs), (got, want)
            if rows is not None:                                     # a full window: the table rows it reads are its recordings' speakers
                assert torch.equal(rows, table[want][:, :4]), recs
    assert not same.per_recording_ids and [ids for ids, _n, _r in equal] == [[1] * len(m) for m in members]


class _StubRunner:
    """Stands in for a `RecordingRunner`: remembers the set it was handed and returns arrays of each recording's length."""
    device = "cpu"

    def __call__(self, rs):
        self.seen = rs
        return [tuple(np.zeros((t, w), np.float32) for _n, w in R.WIDTHS) for t in rs.frames]


def test_test_pass_and_generate_folder_pass_ids_through(tmp_path):
    import json

    import clip_store_common as cc
    _recordings, _clips, index = cc.make_recordings(path=str(tmp_path))
    items = json.load(open(index))
    for it in items:
        rec = os.path.splitext(os.path.basename(it["motion_path"]))[0]
        it["video_id"] = f"{ {'rec0': 4, 'rec1': 2, 'rec2': 7}[rec] }_{it['video_id']}"
        it["mode"] = "test"
    smap = data.SpeakerMap.from_index(items)
    stub = _StubRunner()
    test_list, _save = R.test_pass(None, None, items, str(tmp_path / "out"), runner=stub, speakers=smap)
    assert stub.seen.speaker_ids.tolist() == [smap(it) for it in test_list] and set(stub.seen.speaker_ids.tolist()) == {0, 1, 2}
    R.test_pass(None, None, items, str(tmp_path / "out"), runner=stub)
    assert stub.seen.speaker_ids is None                              # the reference's pass names no speakers
    folder = str(tmp_path / "wave16k")
    R.generate_folder(None, None, folder, str(tmp_path / "gen"), runner=stub)
    assert stub.seen.speaker_ids is None and len(stub.seen) == 3
    R.generate_folder(None, None, folder, str(tmp_path / "gen"), runner=stub, speaker_id=2)
    assert stub.seen.speaker_ids.tolist() == [2, 2, 2]
    R.generate_folder(None, None, folder, str(tmp_path / "gen"), runner=stub, speaker_id=lambda p: int(os.path.basename(p)[3]))
    assert stub.seen.speaker_ids.tolist() == [0, 1, 2]               # rec0.wav, rec1.wav, rec2.wav
