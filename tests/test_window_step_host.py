"""The one window step (`EmageAudioModel._window_step`) and what was folded around it, without a device:
* the op sequence of its three callers — `infer_codes`, the eager `RecordingRunner` pass, the five-session stream scenario — is the one
  recorded in tests/golden/call_logs.json on the commit before the step existed (tests/golden/make_call_logs.py), so the launch sequence
  and the captured graphs did not move;
* `collect_health()` restores `health_pending` on any exit and refuses to nest;
* the step itself over the CPU stand-ins: its seed against a full-length decode of the same codes with `seed_only_decode` both ways, no
  decode without `need_seed`, one health flush between the code ops and the decode ops;
* `windows.split_length` against `window_schedule` and `streaming.tail_of`."""
import json
import os

import pytest
import torch

import call_log_cases
import common
import fake_ops
from pantomatrix_amd import streaming, synthetic, windows
from test_window_schedule import LENGTHS


# ---- same launches -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(call_log_cases.WORKLOADS))
def test_op_sequence_is_the_recorded_one(golden_dir, name):
    with open(os.path.join(golden_dir, "call_logs.json")) as f:
        want = json.load(f)
    assert sorted(want) == sorted(call_log_cases.WORKLOADS)
    got = call_log_cases.digest(call_log_cases.calls_of(name))
    assert got["counts"] == want[name]["counts"] and got["n"] == want[name]["n"]
    assert got["sha256"] == want[name]["sha256"], f"{name}: the same ops in another order"


# ---- collect_health ------------------------------------------------------------------------------------------------------------------------
def test_collect_health_restores_none_and_does_not_nest():
    model, _vq = common.product_models(precision="fp32")
    assert model.health_pending is None
    with pytest.raises(KeyError):
        with model.collect_health() as pending:
            assert model.health_pending is pending and pending == []
            raise KeyError("a body that raises")
    assert model.health_pending is None
    with model.collect_health() as outer:
        with pytest.raises(RuntimeError, match="do not nest"):
            with model.collect_health():
                pass
        assert model.health_pending is outer            # the refused inner block did not touch the outer one's list
    assert model.health_pending is None


# ---- the step ------------------------------------------------------------------------------------------------------------------------------
COL0 = 5                                                 # the window's columns start here in the code buffers: an offset the step must honour


@pytest.fixture(scope="module")
def models():
    """The CPU models, their operand sets packed by one small step: the ops a test logs afterwards are those of the step alone."""
    model, vq = common.product_models(precision="fp32")
    with fake_ops.installed(), torch.no_grad():
        _step(model, vq, 9, need_seed=True)
    return model, vq


def _step(model, vq, t, need_seed, counter=None):
    """One step at B = 2 on fresh code buffers -> (seed, codes, ops logged)."""
    audio = synthetic.synthetic_audio(2, t * windows.SPF, seed=1234)
    spk = torch.zeros(2, 1, dtype=torch.long)
    motion = windows.identity_seed(2, t)
    codes = {p: torch.full((2, COL0 + t + 3), -1, dtype=torch.int64) for p, r in model._routes().items() if r}
    fake_ops.CALLS.clear()
    seed = model._window_step(vq, audio, spk, motion, torch.ones_like(motion), windows.identity_seed(2), codes, COL0, need_seed, counter=counter)
    return seed, codes, list(fake_ops.CALLS)


@pytest.mark.parametrize("t", [64, 40, 9])               # a full window, a tail, and 9 = 4 + 5: the shortest tail the schedule produces
def test_window_step_seed_codes_and_health_flush(models, t):
    model, vq = models
    assert windows.split_length(9)[2] == 9 and windows.split_length(8)[2] == 0
    with fake_ops.installed(), torch.no_grad():
        none, codes, code_ops = _step(model, vq, t, need_seed=False)
        assert none is None and "count_nonfinite_multi" not in code_ops and "count_nonfinite" not in code_ops
        for v in codes.values():                         # the window's columns, and only those
            assert bool((v[:, COL0:COL0 + t] >= 0).all()) and bool((v[:, :COL0] == -1).all()) and bool((v[:, COL0 + t:] == -1).all())
        sel = {f"{p}_index": v[:, COL0:COL0 + t] for p, v in codes.items()}
        full = vq.decode(**sel)["all_motion4inference"]
        assert full.shape == (2, t, 337)
        ts = model._seed_decode_frames(vq, t)
        assert ts == min(t, 4 + 7)
        fake_ops.CALLS.clear()
        vq.decode(**{k: v[:, t - ts:] for k, v in sel.items()})
        short_ops = list(fake_ops.CALLS)
        fake_ops.CALLS.clear()
        vq.decode(**sel)
        full_ops = list(fake_ops.CALLS)
        try:
            for only, decode_ops in ((True, short_ops), (False, full_ops)):
                model.seed_only_decode = only
                seed, again, ops_seen = _step(model, vq, t, need_seed=True)
                assert all(torch.equal(again[p], codes[p]) for p in codes)
                assert seed.shape == (2, 4, 337) and torch.equal(seed, full[:, t - 4:]), (t, only)
                assert ops_seen == code_ops + decode_ops                                # need_seed=False above logged no decode op
                # with a counter, inside collect_health(): ONE flush, between the code ops and the decode ops
                counter = torch.zeros(1, dtype=torch.int32)
                with model.collect_health() as pending:
                    seed, _again, ops_seen = _step(model, vq, t, need_seed=True, counter=counter)
                    assert pending == []                                                # flushed: the next window starts a new list
                assert ops_seen == code_ops + ["count_nonfinite_multi"] + decode_ops and int(counter) == 0
                assert torch.equal(seed, full[:, t - 4:])
        finally:
            model.seed_only_decode = True


# ---- the split of a length -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames", sorted(set(LENGTHS) | set(range(1, 9))))
def test_split_length_agrees_with_the_schedule_and_the_stream(frames):
    rounds, remain, tail = windows.split_length(frames)
    assert (rounds, remain) == ((frames - 4) // 60, (frames - 4) % 60) and tail == (4 + remain if remain > 4 else 0)
    n = synthetic.samples_for_frames(frames)
    assert windows.frames_of(n) == frames
    if frames <= 4:
        assert streaming.tail_of(n) == (0, 0)
        with pytest.raises(ValueError):
            windows.window_schedule([frames])
        return
    assert streaming.tail_of(n) == (rounds, tail)
    s = windows.window_schedule([frames])
    assert (s.rounds, s.remain, s.frames) == ([rounds], [remain], [60 * rounds + tail])
    assert s.tails == ({tail: [(0, 60 * rounds)]} if tail else {}) and len(s.steps) == rounds
