"""Motion hints in live stream sessions, without a device (pantomatrix_amd/streaming.py rule 5 over the stand-ins of
tests/fake_stream_hint_ops.py):
* the five-session scenario, every session hinted with the hints of tests/golden/infer_hints_*.npz, against the eager B = 1
  `model.inference(masked_motion, mask)` + decode under the same stand-ins and against the reference's goldens;
* rule 5's gating (`ready`, `waiting`, `end_motion`, `close()` with a window pending) and the ring's capacity;
* a plain session in a hinted batch, and a batch with motion_hints=False against the op sequence of the scenario's call log;
* `ops.stream_hint_table`'s host checks, and the stand-in's ring arithmetic against dense arrays."""
import numpy as np
import pytest
import torch

import call_log_cases
import common
import fake_hint_ops
import fake_ops
import fake_stream_hint_ops as fh
import stream_common as sc
import stream_hints_common as shc
from pantomatrix_amd import ops, streaming


@pytest.fixture(scope="module")
def models():
    return common.product_models(precision="fp32")


def make_batch(models, **kw):
    with fh.installed(), torch.no_grad():
        return streaming.StreamBatch(*models, slots=3, max_seconds=11, use_graph=False, **kw)


@pytest.fixture(scope="module")
def batch(models):
    """One eager hinted 3-slot batch on the CPU models; max_hint_push = 90 gives a ring of 180 rows (+ 4 mirror rows)."""
    sb = make_batch(models, motion_hints=True, max_hint_push=90)
    assert sb.hint_rows == 180 and tuple(sb.hint_ring_motion.shape) == (3, 184, 344) and sb.hint_ring_keep.dtype == torch.uint8
    assert streaming.StreamBatch.__init__.__defaults__[-2:] == (False, 90)
    return sb


@pytest.fixture(scope="module")
def hinted(batch, golden_dir):
    """The hinted scenario, once -> (results, sessions, calls)."""
    hints = shc.golden_hints(golden_dir)
    assert {k: shc.hint_length(v) for k, v in hints.items()} == shc.HINT_FRAMES
    with fh.installed(), torch.no_grad():
        fake_ops.CALLS.clear()
        got, sessions = shc.scenario(batch, sc.waves(), hints)
        calls = list(fake_ops.CALLS)
    return got, sessions, calls, hints


# ---- the scenario ------------------------------------------------------------------------------------------------------------------------
def test_hinted_sessions_equal_the_eager_hinted_inference(models, hinted):
    model, vq = models
    got, sessions, calls, hints = hinted
    assert "pack_motion" not in calls and calls.count("stream_push_hints") == 5 + 2          # the ticks; the closes of E and C upload hints
    assert calls.count("pack_motion_hints") == 5 + 4                                         # the ticks; the tails of A, B, C and E
    assert [sessions[k].hint_frames_unused for k in "ABCDE"] == [0, 0, 0, 0, 0]
    w = sc.waves()
    spk = torch.zeros(1, 1, dtype=torch.long)
    as_t = lambda a: None if a is None else torch.from_numpy(np.asarray(a, np.float32))[None]
    with fake_hint_ops.installed(), torch.no_grad():
        for name in "ABCDE":
            motion, mask = hints[name]
            lat = model.inference(torch.from_numpy(w[name])[None], spk, vq, masked_motion=as_t(motion), mask=as_t(mask))
            sel = model._select_codes(lat)
            pred = vq.decode(**sel, get_global_motion=True, ref_trans=torch.zeros(1, 3))
            poses, expressions, trans, codes = got[name]
            for p in ("upper", "hands", "lower"):
                assert np.array_equal(codes[p], sel[f"{p}_index"][0].numpy()), (name, p)
            for nm, x, key in (("poses", poses, "motion_axis_angle"), ("expressions", expressions, "expression"), ("trans", trans, "trans")):
                err = float(np.abs(x - pred[key][0].numpy()).max())
                assert x.shape[0] == sc.FRAMES_OUT[name] and err < sc.TOL, (name, nm, err)


def test_hinted_sessions_match_the_reference_goldens(hinted, golden_dir):
    got = hinted[0]
    for name in "ABCDE":
        shc.check_against_golden(name, got[name], golden_dir, "host fp32")
    plain = np.load(f"{golden_dir}/infer_129f_b1.npz")                                       # B: motion=True, no hints, ended at once
    for p in sc.PARTS:
        assert np.array_equal(got["B"][3][p], plain[f"index_{p}"][0]), p


def test_plain_sessions_in_a_hinted_batch_and_the_call_log(models, batch, hinted):
    """The scenario with plain sessions: in a batch built with motion_hints=False it logs the op sequence of the call log's workload (run
    here, in this process); in the hinted batch the same sequence with one `stream_push_hints` a tick and the packing launch exchanged, and
    the same bits."""
    want_calls = call_log_cases.calls_of("stream_five_sessions")
    plain = make_batch(models, motion_hints=False)
    assert not hasattr(plain, "hint_ring_motion") and not hasattr(plain, "hint_staged_host")
    with fh.installed(), torch.no_grad():
        fake_ops.CALLS.clear()
        want = sc.scenario(plain, sc.waves())
        calls = list(fake_ops.CALLS)
        fake_ops.CALLS.clear()
        got = sc.scenario(batch, sc.waves())                                                # slots that held hinted sessions before
        hinted_calls = list(fake_ops.CALLS)
    assert calls == want_calls and "stream_push_hints" not in calls and "pack_motion_hints" not in calls
    assert hinted_calls.count("stream_push_hints") == 5 and hinted_calls.count("pack_motion_hints") == 5
    assert [c.replace("pack_motion_hints", "pack_motion") for c in hinted_calls if c != "stream_push_hints"] == calls
    for name in "ABCDE":
        assert all(np.array_equal(x, y) for x, y in zip(got[name][:3], want[name][:3])), name
        assert all(np.array_equal(got[name][3][p], want[name][3][p]) for p in sc.PARTS), name
    assert any(not np.array_equal(hinted[0]["A"][3][p], want["A"][3][p]) for p in ("upper", "hands", "lower"))      # the hints did something


# ---- rule 5: gating and capacity -------------------------------------------------------------------------------------------------------------
def test_a_window_waits_for_its_hint_frames(batch, monkeypatch):
    monkeypatch.setattr(batch, "_tick", lambda: None)
    monkeypatch.setattr(batch, "_finish", lambda s, rounds, t: None)
    zeros = lambda n: np.zeros(n, dtype=np.float32)
    ident = np.tile(np.array([1.0, 0, 0, 0, 1, 0] * 55 + [0.0] * 7, dtype=np.float32), (200, 1))
    keep = np.zeros((200, 337), np.uint8)
    with fh.installed():
        s = batch.open(motion=True)
        assert s.waiting == "audio" and not s.ready
        s.push(zeros(streaming.window_need(0)))
        assert s.waiting == "motion" and not s.ready and batch.step() == {}
        s.push_motion(ident[:63], keep[:63])
        assert s.waiting == "motion" and batch.step() == {} and s.hint_frames == 63
        s.push_motion(mask=keep[:1])                                                # the 64th frame, a mask alone
        assert s.waiting is None and s.ready and list(batch.step()) == [s] and s.windows == 1
        s.push(zeros(streaming.window_need(1) - s.pushed))
        assert s.waiting == "motion"                                                # window 1 needs frames up to 124
        with pytest.raises(RuntimeError, match="pending"):
            s.close()                                                               # close() ends the hints: the window is pending, as for audio
        assert s.hints_ended and s.waiting is None
        with pytest.raises(RuntimeError, match="ended"):
            s.push_motion(ident[:1])
        assert list(batch.step()) == [s] and s.windows == 2
        s.close()
        assert s.waiting is None and s.hint_frames_unused == 0
        # end_motion() releases a waiting window too, and is idempotent; hints beyond the frames produced are counted
        s = batch.open(motion=True)
        s.push(zeros(streaming.window_need(0)))
        s.push_motion(ident[:70])
        assert s.ready
        s.end_motion(), s.end_motion()
        assert list(batch.step()) == [s]
        s.close()                                                                   # 64 frames of audio: 60 frames out, no tail
        assert s.emitted == 60 and s.hint_frames_unused == 10
        with pytest.raises(RuntimeError):
            s.end_motion()


def test_pushes_that_do_not_fit_or_do_not_parse_raise(models, batch, monkeypatch):
    monkeypatch.setattr(batch, "_tick", lambda: None)
    monkeypatch.setattr(batch, "_finish", lambda s, rounds, t: None)
    ident = np.tile(np.array([1.0, 0, 0, 0, 1, 0] * 55 + [0.0] * 7, dtype=np.float32), (200, 1))
    with fh.installed():
        with pytest.raises(ValueError, match="not both"):
            batch.open(seed=torch.zeros(4, 337), motion=True)
        with pytest.raises(ValueError, match="motion_hints=True"):
            make_batch(models).open(motion=True)
        assert batch.sessions == [None] * 3
        s, plain = batch.open(motion=True), batch.open()
        with pytest.raises(RuntimeError):
            plain.push_motion(ident[:1])
        s.push_motion(ident[:2])
        with pytest.raises(ValueError, match="do not mix"):
            s.push_motion(poses=np.zeros((1, 165), np.float32))                     # packed frames are staged for the next tick
        s.push_motion(ident[:178])                                                  # the whole ring
        with pytest.raises(ValueError, match="do not fit"):
            s.push_motion(ident[:1])
        s.push(np.zeros(streaming.window_need(0), dtype=np.float32))
        assert list(batch.step()) == [s]
        s.push_motion(ident[:60])                                                   # one window on: 60 more rows are free
        with pytest.raises(ValueError, match="do not fit"):
            s.push_motion(ident[:1])
        for bad in (dict(motion=ident[:2, :336]), dict(motion=ident[:2], mask=np.ones((3, 337))), dict(mask=np.full((2, 337), 0.5)),
                    dict(mask=np.full((2, 337), 2)), dict(mask=np.full((2, 337), np.nan)), dict(motion=ident[:2], poses=np.zeros((2, 165))),
                    dict(trans=np.zeros((2, 3))), dict(poses=np.zeros((2, 165)), contact=np.zeros((2, 3))), dict()):
            with pytest.raises(ValueError):
                s.push_motion(**bad)
        s._hint_staged, s._staged = [], []
        s.close(), plain.close()


# ---- the table builder and the stand-in's rings --------------------------------------------------------------------------------------------
GEOMETRY = dict(hint_rows=120, staged_bytes=3 * ops.stream_hint_chunk_bytes(64, 0))


def test_stream_hint_table_checks_what_it_builds():
    chunk = ops.stream_hint_chunk_bytes(64, 0)
    assert chunk == 107840 and ops.stream_hint_chunk_bytes(7, 1) == 7184 and chunk % 16 == 0
    tab = ops.stream_hint_table([dict(frames=64, src=0, form=0, frames_before=0, ready=1, window_index=0), None,
                                 dict(frames=7, src=chunk, form=1, frames_before=118), dict(frames_before=130, ready=1, window_index=2),
                                 dict(frames=2, src=2 * chunk, frames_before=2)], **GEOMETRY)
    assert tab.dtype == np.int32 and tab.shape == (5, ops.STREAM_HINT_WORDS) and not tab[1].any()
    assert tab[0].tolist()[:9] == [64, 0, 0, 0, 0, 4, 1, 0, 64]
    assert tab[2].tolist()[:9] == [7, chunk // 16, 1, 118, 0, 0, 0, 0, 0]
    assert tab[3].tolist()[:9] == [0, 0, 0, 10, 0, 0, 1, 0, 10]                     # window 2 of a 120-row ring starts at row 0; 130 - 120 frames
    assert tab[4].tolist()[:9] == [2, 2 * chunk // 16, 0, 2, 2, 2, 0, 0, 0]
    for bad in (dict(frames=121, src=0), dict(frames=64, src=8), dict(frames=64, src=2 * chunk + 16), dict(frames=1, src=0, form=2),
                dict(frames=1, src=0, frames_before=-1), dict(frames=-1), dict(ready=1, window_index=-1), dict(frames_before=241, ready=1, window_index=2),
                dict(frames=1, src=0, push=3)):
        with pytest.raises(ValueError):
            ops.stream_hint_table([bad], **GEOMETRY)
    with pytest.raises(ValueError):
        ops.stream_hint_table([dict(frames=64, src=0), dict(frames=1, src=chunk - 16)], **GEOMETRY)         # two chunks overlap
    with pytest.raises(ValueError):
        ops.stream_hint_table([None], hint_rows=100, staged_bytes=16)


def test_stand_in_ring_keeps_every_window_contiguous():
    """Pushes of 7 frames into the smallest ring: after every push the 64 rows from (60 i) % 120 of the last complete window equal the
    dense frames, the mirror rows included; the seed rows take frames 0 .. 3 only."""
    rng = np.random.default_rng(3)
    frames = rng.standard_normal((400, 337)).astype(np.float32)
    keep = rng.integers(0, 2, (400, 337)).astype(np.uint8)
    ring_m, ring_k = np.full((2, 124, 344), -7.0, np.float32), np.full((2, 124, 344), 9, np.uint8)
    seeds, wt = np.full((2, 4, 337), -7.0, np.float32), np.full((2, 2), -1, np.int64)
    for lo in range(0, 399, 7):
        n = min(7, 399 - lo)
        i = (lo + n - 64) // 60 if lo + n >= 64 else None                           # the window this push completes, if it completes one
        if i is not None and 60 * i + 64 <= lo:
            i = None
        staged, (at,) = fh.stage([(0, frames[lo:lo + n], keep[lo:lo + n])])
        row = dict(frames=n, src=at, frames_before=lo, **({} if i is None else dict(ready=1, window_index=i)))
        tab = ops.stream_hint_table([None, row], hint_rows=120, staged_bytes=staged.size)
        assert fh.ring_model(staged, tab, ring_m, ring_k, seeds, wt, 64) == 0
        assert wt[0].tolist() == [0, 0]
        if i is not None:
            first, avail = wt[1].tolist()
            assert first == 124 + (60 * i) % 120 and avail == 64
            got_m, got_k = ring_m.reshape(-1, 344)[first:first + 64], ring_k.reshape(-1, 344)[first:first + 64]
            assert np.array_equal(got_m[:, :337], frames[60 * i:60 * i + 64]) and np.array_equal(got_k[:, :337], keep[60 * i:60 * i + 64])
            assert not got_m[:, 337:].any() and (got_k[:, 337:] == 1).all()
    assert np.array_equal(seeds[1], frames[:4]) and (seeds[0] == -7.0).all() and (ring_m[0] == -7.0).all()
