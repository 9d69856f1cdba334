"""Host side of the ragged DisCo / CaMN pass (recordings of different lengths as one batch): the CPU restatement of the lengths
recurrence, the planning logic of pantomatrix_amd/lstm_recordings.py, the error messages, `forward_ragged` with every C-ABI call replaced
by its torch restatement, and the golden fixture against the oracle.  The kernel and the runner are tested on the MI355X in
tests/test_lstm_ragged_gpu.py."""
import os

import numpy as np
import pytest
import torch

import fake_lstm_ragged_ops as ragged_fake
import fake_ops
from pantomatrix_amd import lstm_recordings as LR
from pantomatrix_amd import modeling_lstm_audio as L
from pantomatrix_amd._lib import F16X3
from test_lstm_models_oracle import CFG, weights, run_oracle
from tools.workloads import lstm_product as product

# three recordings whose frame counts differ (34 / 28 / 36); the first has odd frame counts behind WavEncoder blocks 0-2 (7891 / 1313 /
# 1313: the padded route), the other two even ones (the pair-rows route) — both routes in one batch
RAGGED_SAMPLES = (36266, 30000, 38400)
RAGGED_FRAMES = (34, 28, 36)
# The waveforms.  With the synthetic weights a tenth of all joints come out within 0.14 rad of a half turn, where the reference's own
# rot-6D -> axis-angle conversion magnifies float32 rounding a few thousand times: the ORACLE in float32 against itself in float64 (the
# reference's arithmetic, no product code involved) differs by 1.5e-7 in rot-6D on every input but by up to 1.2e-3 in axis-angle on
# some — more than the whole 1e-3 axis-angle bar the reference comparisons use.  So the noise seed is the first one from 11 on at which
# that own error stays within a quarter of the bar (2.5e-4) in all six outputs (tests/golden/make_golden_lstm_recordings.py computes and
# asserts it): largest own error per seed 11: 5.7e-4, 12: 2.8e-4, 13: 1.1e-3, 14: 5.5e-4, 15: 1.2e-3, 16: 4.0e-4, 17: 2.0e-4.
RAGGED_SEED = 17
OWN_ERROR_SHARE = 0.25


def ragged_inputs(seed=RAGGED_SEED):
    g = torch.Generator().manual_seed(seed)
    audios = [0.1 * torch.randn(n, generator=g) for n in RAGGED_SAMPLES]
    return audios, torch.zeros(len(audios), dtype=torch.long)       # speaker_dims = 1: the one speaker of the synthetic checkpoint


def test_fake_lengths_recurrence_equals_each_clip_alone():
    """The restatement the host tests run the model on: masked state forced to zero == every clip alone over its own length, although
    gates_x is NaN past each clip's end."""
    hid, b, t = 256, 5, 7
    lengths = [7, 1, 4, 7, 2]
    g = torch.Generator().manual_seed(2)
    gx = torch.randn(b, t, 8 * hid, generator=g)
    w = [(0.05 * torch.randn(4 * hid, hid, generator=g)) for _ in range(2)]
    packed = [fake_ops_pack(x) for x in w]
    for k, l in enumerate(lengths):
        gx[k, l:] = float("nan")
    hseq = torch.full((b, t, 2 * hid), float("nan"))
    sync = fake_ops.lstm_layer_sync(b, hid, "cpu")
    ragged_fake.lstm_layer(F16X3, gx, [p[0] for p in packed], [p[1] for p in packed], hseq, sync, lengths=torch.tensor(lengths, dtype=torch.int32))
    for k, l in enumerate(lengths):
        alone = torch.empty(1, l, 2 * hid)
        fake_ops.lstm_layer(F16X3, gx[k:k + 1, :l].contiguous(), [p[0] for p in packed], [p[1] for p in packed], alone, sync)
        assert torch.equal(hseq[k, :l], alone[0]), k
        assert not hseq[k, l:].any()
    full = torch.empty(b, t, 2 * hid)
    clean = torch.nan_to_num(gx)
    ragged_fake.lstm_layer(F16X3, clean, [p[0] for p in packed], [p[1] for p in packed], full, sync, lengths=torch.full((b,), t, dtype=torch.int32))
    plain = torch.empty(b, t, 2 * hid)
    fake_ops.lstm_layer(F16X3, clean, [p[0] for p in packed], [p[1] for p in packed], plain, sync)
    assert torch.equal(full, plain)


def fake_ops_pack(w):
    """(packed weight, scale) of a recurrent weight in the product's F16X3 layout, through the product's own packer."""
    from pantomatrix_amd import modeling_emage_audio as M
    pk = M._Packed({}, torch.device("cpu"), F16X3)
    wp, _kp, ws = pk._pack_mat(w)
    return wp, ws


def test_frames_follow_the_wav_encoder():
    model = product("camn")
    assert model.ragged_frames(RAGGED_SAMPLES) == list(RAGGED_FRAMES) == [model._wav_lengths(n)[-1] for n in RAGGED_SAMPLES]
    lens = [model._wav_lengths(n) for n in RAGGED_SAMPLES]
    assert [model._wav_pairs_ok(l) for l in lens] == [False, True, True] and all(x % 2 for x in lens[0][:3])


def test_plan_sorts_and_cuts():
    frames = [30, 90, 30, 45, 120, 31]
    order, batches = LR.plan_batches(frames, 512, max_batch=256)
    assert order == [4, 1, 3, 5, 0, 2] and batches == [order]                 # longest first, ties in input order, one batch
    inverse = {r: k for k, r in enumerate(order)}
    assert sorted(inverse) == list(range(len(frames))) and [order[inverse[r]] for r in range(len(frames))] == list(range(len(frames)))
    assert LR.padded_share(frames, batches) == pytest.approx(1 - sum(frames) / (6 * 120))
    order, batches = LR.plan_batches(frames, 512, max_batch=4)
    assert batches == [[4, 1, 3, 5], [0, 2]] and sum(batches, []) == order
    assert LR.padded_share(frames, batches) == pytest.approx(1 - sum(frames) / (4 * 120 + 2 * 30))


@pytest.mark.parametrize("hid", [256, 512])
def test_plan_respects_the_operand_span(hid):
    """gates_x of a batch is B * Tmax rows of 8H floats and must stay below 2 GiB: fabricated lengths on both sides of that."""
    t = 1000
    fit = ((1 << 31) - 1) // (t * 8 * hid * 4)                                 # the most recordings of t frames one batch may hold
    assert L.ragged_batch_limit(fit, t, hid) is None
    why = L.ragged_batch_limit(fit + 1, t, hid)
    assert why and str((fit + 1) * t * 8 * hid * 4) in why and str(1 << 31) in why
    frames = [t] * (fit + 1) + [10]
    _order, batches = LR.plan_batches(frames, hid, max_batch=1000)            # (max_batch out of the way: 262 recordings fit at H = 256)
    assert [len(x) for x in batches] == [fit, 2]
    assert all(L.ragged_batch_limit(len(x), max(frames[i] for i in x), hid) is None for x in batches)


def test_plan_refuses_an_over_long_recording():
    """64 clip rows of the (B, Tmax, 2H) layer output are addressed with 32-bit offsets (emage_lstm_layer's own check)."""
    hid = 512
    t_ok = ((1 << 31) - 4096 - 1) // (64 * 2 * hid * 4)
    assert 64 * t_ok * 2 * hid * 4 + 4096 < (1 << 31) <= 64 * (t_ok + 1) * 2 * hid * 4 + 4096
    LR.plan_batches([t_ok, 5], hid)
    with pytest.raises(ValueError, match=rf"recording 1: a recording of {t_ok + 1} frames is too long .* {64 * (t_ok + 1) * 2 * hid * 4 + 4096} bytes"):
        LR.plan_batches([5, t_ok + 1], hid)


def test_error_messages():
    model = product("disco")
    with pytest.raises(ValueError, match="no recordings"):
        LR.plan_batches([], 512)
    with pytest.raises(ValueError, match="no recordings"):
        model.ragged_frames([])
    with pytest.raises(ValueError, match=r"recording 1 has 0 samples, the WavEncoder needs at least 1"):
        model.ragged_frames([36266, 0])
    audios, spk = ragged_inputs()
    with fake_ops.installed():
        with pytest.raises(ValueError, match="3 recordings but 2 speaker ids"):
            model.forward_ragged(audios, spk[:2])
        with pytest.raises(ValueError, match="1-D float waveform"):
            model.forward_ragged([audios[0][None]], spk[:1])
    hid = model.config.hidden_size
    n = ((1 << 31) - 1) // (RAGGED_FRAMES[0] * 8 * hid * 4) + 1              # as many copies of one recording as cross the gates_x limit
    with fake_ops.installed(), pytest.raises(ValueError, match=rf"{n} recordings padded to {RAGGED_FRAMES[0]} frames"):
        model.forward_ragged([audios[0]] * n, torch.zeros(n, dtype=torch.long))


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("kind", ["disco", "camn"])
def test_forward_ragged_matches_each_recording_alone_and_the_golden(golden_dir, kind, precision):
    """The host logic of `forward_ragged` on the CPU restatements: f16x3 takes the lengths recurrence (one call per LSTM layer), fp32 the
    groups of equal frame count; both give each recording what the B = 1 forward gives it, and the reference's result."""
    g = np.load(os.path.join(golden_dir, "lstm_recordings.npz"))
    audios, spk = ragged_inputs()
    model = product(kind, precision)
    with ragged_fake.installed(), torch.no_grad():
        got = model.forward_ragged(audios, spk, seed_frames=CFG["seed_frames"])
        calls = list(fake_ops.CALLS)
        alone = [model(a[None], spk[r].view(1, 1), seed_frames=CFG["seed_frames"]) for r, a in enumerate(audios)]
    n_lstm = (1 if kind == "disco" else 2) * CFG["n_layer"]
    if precision == "f16x3":
        assert calls.count("lstm_layer_lengths") == n_lstm and "lstm_step_pair" not in calls and "lstm_layer" not in calls
    else:
        assert calls.count("lstm_step_pair") == n_lstm * sum(RAGGED_FRAMES) and "lstm_layer_lengths" not in calls
    assert calls.count("wav_conv_in") == 1 + 2 + 2                              # the padded route once, the pair-rows route twice
    for r, t in enumerate(RAGGED_FRAMES):
        assert set(got[r]) == set(alone[r])
        for k, v in got[r].items():
            assert v.shape == alone[r][k].shape[1:] and v.shape[0] == t
            assert float((v - alone[r][k][0]).abs().max()) < 1e-4, (r, k)
        np.testing.assert_allclose(got[r]["motion"].reshape(t, -1).numpy(), g[f"{kind}_{r}_motion"], atol=5e-5, rtol=0)
        np.testing.assert_allclose(got[r]["motion_axis_angle"].numpy(), g[f"{kind}_{r}_axis_angle"], atol=1e-3, rtol=0)


def test_oracle_matches_golden(golden_dir):
    """Pins the fixture: the oracle on each recording alone gives the reference modules' recorded outputs."""
    g = np.load(os.path.join(golden_dir, "lstm_recordings.npz"))
    audios, spk = ragged_inputs()
    assert sorted(g.files) == sorted(f"{kind}_{r}_{k}" for kind in ("disco", "camn") for r in range(3) for k in ("motion", "axis_angle"))
    for kind in ("disco", "camn"):
        for r, (audio, t) in enumerate(zip(audios, RAGGED_FRAMES)):
            got = run_oracle(kind, weights(kind), audio[None], spk[r].view(1, 1), None)
            assert g[f"{kind}_{r}_motion"].shape == (t, CFG["pose_dims"]) and g[f"{kind}_{r}_axis_angle"].shape == (t, 165)
            np.testing.assert_allclose(got["motion"].reshape(t, -1).numpy(), g[f"{kind}_{r}_motion"], atol=2e-5, rtol=0)
            np.testing.assert_allclose(got["motion_axis_angle"].reshape(t, 165).numpy(), g[f"{kind}_{r}_axis_angle"], atol=1e-3, rtol=0)
