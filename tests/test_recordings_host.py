"""The lock-step test pass without a device: `recordings.window_schedule` against a per-recording restatement of the reference's window
arithmetic (models/emage_audio/modeling_emage_audio.py:364-368, 380-382, 428-431), `RecordingSet.from_index` over the files the reference's
dataset reads, the host check of a copy-segment table, and the file naming / npz schema of `test_pass` over a stub runner."""
import json
import os

import numpy as np
import pytest
import torch

import clip_store_common as cc
from oracle import emage_oracle as orc
from pantomatrix_amd import data, motion_io, ops, recordings as R

EDGE_LENGTHS = (63, 64, 68, 69, 124, 128)
SHUFFLED = [70, 310, 40, 129, 64, 63, 188, 9, 68, 69, 124, 128]        # 12 lengths, a fixed shuffle: every case, equal tails at different starts


def reference_windows(total_len, window=64, pre_frames=4):
    """What M:364-368 / M:380-382 / M:428-431 run for ONE recording -> [(start, end, frames kept)]."""
    rounds = (total_len - pre_frames) // (window - pre_frames)
    remain = (total_len - pre_frames) % (window - pre_frames)
    out = []
    for i in range(rounds):
        start_idx = i * (window - pre_frames)
        out.append((start_idx, start_idx + window, window - pre_frames))           # M:419 `[:, :-pre_frames]`
    if remain > pre_frames:
        final_start = rounds * (window - pre_frames)
        out.append((final_start, final_start + pre_frames + remain, pre_frames + remain))
    return out


def schedule_windows(s, k):
    """The windows a `Schedule` gives recording k, in running order."""
    out = [(start, start + s.window, s.window - s.seed_frames) for start, ids in s.steps if k in ids]
    for t, members in s.tails.items():
        out += [(start, start + t, t) for r, start in members if r == k]
    return out


def check(lengths):
    s = R.window_schedule(lengths)
    for k, t in enumerate(lengths):
        want = reference_windows(t)
        assert schedule_windows(s, k) == want, (t, schedule_windows(s, k), want)
        assert s.frames[k] == sum(w[2] for w in want), t
        assert s.rounds[k] == (t - 4) // 60 and s.remain[k] == (t - 4) % 60
    for i, (start, ids) in enumerate(s.steps):                                     # one start per step; active sets shrink, never grow
        assert start == 60 * i and ids == [k for k, t in enumerate(lengths) if (t - 4) // 60 > i] and ids
    for t, members in s.tails.items():
        assert 9 <= t <= 63 and all(lengths[r] - start == t for r, start in members)    # a tail ends at its recording's end
    assert s.n_windows == sum(len(reference_windows(t)) for t in lengths)
    return s


@pytest.mark.parametrize("length", range(5, 201))
def test_schedule_of_one_recording(length):
    check([length])


def test_schedule_edge_lengths():
    s = check(list(EDGE_LENGTHS))
    assert s.frames == [63, 60, 60, 69, 120, 120]
    assert s.tails == {63: [(0, 0)], 9: [(3, 60)]}                                 # 64: no tail; 68, 128: remainder of 4 dropped; 124: none left
    assert [ids for _s, ids in s.steps] == [[1, 2, 3, 4, 5], [4, 5]]


def test_schedule_of_a_shuffled_list():
    s = check(SHUFFLED)
    assert s.tails[10] == [(0, 60), (1, 300)]                                      # 70 and 310: the same tail length at different starts
    assert [len(ids) for _s, ids in s.steps] == [9, 5, 2, 1, 1]
    assert R.window_schedule([8]).frames == [0] and R.window_schedule([5]).tails == {}
    with pytest.raises(ValueError):
        R.window_schedule([70, 4])


def test_segment_table_refuses_overlap_and_out_of_range():
    tab, longest = ops.segment_table([(0, 5, 3), (3, 0, 5)], 8, 8)
    assert tab.dtype == np.int64 and tab.shape == (2, 3) and longest == 5
    with pytest.raises(ValueError):
        ops.segment_table([(0, 0, 3), (3, 2, 3)], 8, 8)                            # destinations [0, 3) and [2, 5)
    with pytest.raises(ValueError):
        ops.segment_table([(6, 0, 3)], 8, 8)                                       # source rows [6, 9) of 8
    with pytest.raises(ValueError):
        ops.segment_table([(0, 2, 3)], 8, 8, same_buffer=True)                     # in place: destination [2, 5) over source [0, 3)
    ops.segment_table([(0, 4, 3), (0, 1, 3)], 8, 8, same_buffer=False)             # sources may repeat


@pytest.fixture()
def test_split(tmp_path):
    """The three recordings of the clip-store fixture as files, with an index of our own: two test recordings (one named twice, one
    of them behind a train item), one train-only recording."""
    recordings, clips, _index = cc.make_recordings(path=str(tmp_path))
    p = lambda r: dict(motion_path=str(tmp_path / "smplxflame_30" / f"rec{r}.npz"), audio_path=str(tmp_path / "wave16k" / f"rec{r}.wav"))
    items = [dict(video_id="a", mode="test", start_idx=0, end_idx=8, **p(0)),
             dict(video_id="c", mode="train", start_idx=0, end_idx=8, **p(2)),
             dict(video_id="a", mode="test", start_idx=3, end_idx=11, **p(0)),
             dict(video_id="b", mode="test", start_idx=0, end_idx=8, **p(1)),
             dict(video_id="b", mode="train", start_idx=0, end_idx=8, **p(1))]
    index = str(tmp_path / "test_index.json")
    with open(index, "w") as f:
        json.dump(items, f)
    return recordings, clips, index, items


def test_from_index_filters_dedupes_and_keeps_raw_poses(test_split):
    recordings, clips, index, items = test_split
    rs = R.RecordingSet.from_index(index, "test", "cpu")
    assert [it["video_id"] for it in rs.items] == ["a", "b"] and rs.items[0] == items[0] and rs.items[1] == items[3]      # first per video_id
    assert len(rs) == 2 and rs.seeded and rs.audio_format == "int16" and rs.audio.dtype == torch.int16
    assert rs.sample_counts == [len(recordings[0]["audio"]), len(recordings[1]["audio"])] and rs.frames == [19, 26]      # M:345: 27 * 533 + 7 samples are 26 frames
    assert torch.equal(rs.audio, torch.from_numpy(np.concatenate([recordings[0]["audio"], recordings[1]["audio"]])))
    store = data.ClipStore.from_arrays(recordings, clips, "cpu")
    for k, r in enumerate((0, 1)):
        rec = recordings[r]
        raw = torch.from_numpy(rec["poses"][:4])
        assert torch.equal(rs.seed_poses[k], raw)
        assert not torch.equal(rs.seed_poses[k], torch.from_numpy(store.recordings[r]["poses"][:4]))      # the store's are normalised, x / (1 + 1e-7)
        want = torch.cat([orc.axis_angle_to_rotation_6d(raw.reshape(4, 55, 3)).reshape(4, 330), torch.from_numpy(rec["trans"][:4]),
                          torch.from_numpy(rec["foot_contact"][:4])], dim=-1)
        assert rs.seeds[k].shape == (4, 337) and torch.allclose(rs.seeds[k], want, rtol=0, atol=1e-6)
        assert torch.equal(rs.ref_trans[k], torch.from_numpy(rec["trans"][0]))
    for source in ([index], items):
        again = R.RecordingSet.from_index(source, "test", "cpu")
        assert torch.equal(again.audio, rs.audio) and torch.equal(again.seeds, rs.seeds)
    with pytest.raises(ValueError):
        R.RecordingSet.from_index(index, "val", "cpu")


def test_from_audio_has_identity_seed_and_float32_for_mixed_input(test_split, tmp_path):
    recordings, _clips, _index, items = test_split
    rs = R.RecordingSet.from_audio([items[0]["audio_path"], recordings[1]["audio"].astype(np.float32) / 32768.0], "cpu")
    assert not rs.seeded and rs.audio_format == "float32" and rs.items is None
    want = np.concatenate([recordings[0]["audio"], recordings[1]["audio"]]).astype(np.float32) / np.float32(32768.0)
    assert torch.equal(rs.audio, torch.from_numpy(want))
    ident = torch.tensor([1.0, 0, 0, 0, 1, 0] * 55 + [0.0] * 7)
    assert torch.equal(rs.seeds, ident.expand(2, 4, 337)) and torch.equal(rs.ref_trans, torch.zeros(2, 3))
    assert torch.equal(orc.axis_angle_to_rotation_6d(torch.zeros(55, 3)).reshape(-1), ident[:330])      # M:348-349: the reference's default


def test_runner_host_logic_matches_the_reference_goldens(golden_dir):
    """The pass itself over the CPU stand-ins of every kernel: schedule, seed chain, hoisting in chunks, tail groups gathered and
    scattered, per-length decode and packing in input order — against the REFERENCE's B = 1 goldens of the same waveforms.  70 and 310
    frames share the 10-frame tail group at different starts, 40 is tail-only, 64 has no tail; max_batch = 2 splits the first step, max_hoist_rows = 3 the seven full windows into three chunks."""
    import common
    import fake_ops
    import fake_recording_ops
    from pantomatrix_amd import synthetic
    frames, frames_out = (70, 310, 40, 64), (70, 310, 40, 60)
    model, vq = common.product_models(precision="fp32")
    waves = [synthetic.synthetic_audio(1, synthetic.samples_for_frames(f))[0] for f in frames]
    with fake_recording_ops.installed(), torch.no_grad():
        rs = R.RecordingSet.from_audio(waves, "cpu")
        runner = R.RecordingRunner.for_set(model, vq, rs, use_graph=False, max_batch=2, max_hoist_rows=3)
        assert runner.order == [1, 0, 3, 2] and [(u.start, u.lo, u.hi) for u in runner.units] == [(0, 0, 2), (0, 2, 3), (60, 0, 1), (120, 0, 1),
                                                                                                 (180, 0, 1), (240, 0, 1)]
        assert [(s0, n) for s0, n, _u in runner.chunks] == [(0, 3), (3, 3), (6, 1)] and [(g.t, g.n) for g in runner.tails] == [(40, 1), (10, 2)]
        fake_ops.CALLS.clear()
        results = [tuple(a.copy() for a in r) for r in runner(rs)]
        calls = list(fake_ops.CALLS)
        codes = [{p: v.numpy().copy() for p, v in runner.codes_of(k).items()} for k in range(len(frames))]
    assert calls.count("gather_windows") == 3 + 2                               # one per hoisting chunk, one per tail group
    assert calls.count("copy_segments") == 2 * (1 + 4) + 4 * 3                     # per tail group: seeds + four code scatters; per decode group: three outputs
    for k, f in enumerate(frames):
        g = np.load(os.path.join(golden_dir, f"infer_{f}f_b1.npz"))
        for p in ("face", "upper", "hands", "lower"):
            assert np.array_equal(codes[k][p], g[f"index_{p}"][0]), (f, p)
        for nm, got in zip(("poses", "expressions", "trans"), results[k]):
            assert got.shape[0] == frames_out[k] and float(np.abs(got - g[nm][0]).max()) < 1e-3, (f, nm)


class StubRunner:
    """Stands in for a `RecordingRunner`: fixed arrays per recording, T frames of the recording's own length."""
    device = "cpu"

    def __call__(self, rs):
        self.seen = rs
        out = []
        for k, t in enumerate(rs.frames):
            g = np.random.default_rng(100 + k)
            out.append(tuple(g.standard_normal((t, w)).astype(np.float32) for _n, w in R.WIDTHS))
        return out


def test_test_pass_writes_the_reference_files(test_split, tmp_path):
    _recordings, _clips, index, items = test_split
    stub, save = StubRunner(), str(tmp_path / "out")
    test_list, save_list = R.test_pass(None, None, [index], save, runner=stub)
    assert test_list == [items[0], items[3]]
    assert [sorted(e) for e in save_list] == [["audio_path", "motion_path", "video_id"]] * 2
    want = stub(stub.seen)
    for e, it, (poses, expressions, trans) in zip(save_list, test_list, want):
        assert e["video_id"] == it["video_id"] and e["audio_path"] == it["audio_path"]
        assert e["motion_path"] == os.path.join(save, f"{it['video_id']}_output.npz") and os.path.isfile(e["motion_path"])
        z = np.load(e["motion_path"], allow_pickle=True)
        assert sorted(z.files) == ["betas", "expressions", "gender", "mocap_frame_rate", "model", "poses", "trans"]
        assert z["betas"].shape == (300,) and str(z["model"]) == "smplx2020" and str(z["gender"]) == "neutral" and int(z["mocap_frame_rate"]) == 30
        got = motion_io.beat_format_load(e["motion_path"])
        assert np.array_equal(got["poses"], poses) and np.array_equal(got["expressions"], expressions) and np.array_equal(got["trans"], trans)
    assert sorted(os.listdir(save)) == ["a_output.npz", "b_output.npz"]
