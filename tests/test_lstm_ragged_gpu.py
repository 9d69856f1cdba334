"""Recordings of different lengths as one DisCo / CaMN batch, on the MI355X: the persistent recurrence with per-clip lengths
(`ops.lstm_layer(..., lengths=)`, csrc/lstmseq.hip) against the kernel it already is — every clip's valid steps must carry the BITS of
that clip run over its own length —, `forward_ragged` of both models against the B = 1 forward and the REFERENCE's golden outputs
(tests/golden/lstm_recordings.npz), `LstmRecordingRunner` captured against eager, and `generate_folder_lstm` on WAV files."""
import os
import wave

import numpy as np
import pytest
import torch

from pantomatrix_amd import lstm_recordings as LR
from pantomatrix_amd import motion_io, ops
from pantomatrix_amd._lib import F16X3
from pantomatrix_amd.recordings import RecordingSet
from test_lstm_host_logic import product
from test_lstm_models_oracle import CFG
from test_lstm_ragged_host import RAGGED_FRAMES, RAGGED_SAMPLES, ragged_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _lengths_130():
    """A length-1 and a length-5 clip inside one 16-clip fragment; the lengths change across the 32- and the 64-clip slice borders."""
    ln = [1 + (3 * i + i // 32) % 5 for i in range(130)]
    ln[0], ln[1] = 1, 5
    ln[31], ln[32] = 2, 5
    ln[63], ln[64] = 1, 4
    return ln


KERNEL_CASES = [(5, 7, 512, [7, 1, 4, 7, 2]),
                (70, 6, 256, [1 + i % 6 for i in range(70)]),
                (130, 5, 512, _lengths_130()),
                (300, 4, 512, [1 + i % 4 for i in range(300)])]              # two launch records: the lengths pointer advances with the chunk


@pytest.mark.parametrize("b,t,hid,lengths", KERNEL_CASES, ids=[f"B{c[0]}-T{c[1]}-H{c[2]}" for c in KERNEL_CASES])
def test_lengths_kernel_equals_each_length_alone(b, t, hid, lengths):
    g = torch.Generator().manual_seed(b + t)
    wp, ws = [], []
    for _ in range(2):
        p, s = ops.split_f16_weights(torch.randn(4 * hid, hid, generator=g) / hid ** 0.5)
        wp.append(p.to(DEV))
        ws.append(s)
    clean = torch.randn(b, t, 8 * hid, generator=g).to(DEV)
    ln = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    gx = clean.clone()
    gx[torch.arange(t, device=DEV)[None, :] >= ln[:, None]] = float("nan")      # nothing past a clip's end may be used
    sync = ops.lstm_layer_sync(b, hid, DEV)

    def run(gates, **kw):
        hseq = torch.full(gates.shape[:2] + (2 * hid,), float("nan"), device=DEV)
        s = sync if gates.shape[0] == b else ops.lstm_layer_sync(gates.shape[0], hid, DEV)
        ops.lstm_layer(F16X3, gates, wp, ws, hseq, s, **kw)
        torch.cuda.synchronize()
        ops.lstm_layer_check(s)
        return hseq

    out = run(gx, lengths=ln)
    for l in sorted(set(lengths)):
        sel = torch.tensor([i for i, x in enumerate(lengths) if x == l], device=DEV)
        alone = run(gx[sel, :l].contiguous())                                    # the clips of this length as their own batch, no lengths
        assert torch.equal(out[sel, :l], alone), f"length {l}: not the bits of the clips run alone"
        assert not bool(out[sel, l:].any()), f"length {l}: the masked steps are not exactly 0"
    assert torch.equal(run(gx, lengths=ln), out)                                 # a second call on the same buffers repeats the bits
    plain = run(clean)
    assert torch.equal(run(clean, lengths=None), plain)
    assert torch.equal(run(clean, lengths=torch.full((b,), t, dtype=torch.int32, device=DEV)), plain)


def _ragged_on_device():
    audios, spk = ragged_inputs()
    return [a.to(DEV) for a in audios], spk.to(DEV)


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("kind", ["disco", "camn"])
def test_forward_ragged_matches_b1_and_reference(golden_dir, kind, precision):
    """Each recording of the ragged batch against `model(audio_b[None], spk_b)` (bar 1e-4: the clip-independence bar of
    test_baseline_batch_properties) and against the reference modules' outputs (2e-4 rot-6D, 1e-3 axis-angle: the bars of
    test_models_match_reference_golden).  fp32 takes the group-by-length route."""
    g = np.load(os.path.join(golden_dir, "lstm_recordings.npz"))
    audios, spk = _ragged_on_device()
    model = product(kind, precision, DEV)
    with torch.no_grad():
        got = model.forward_ragged(audios, spk, seed_frames=CFG["seed_frames"])
        for r, t in enumerate(RAGGED_FRAMES):
            alone = model(audios[r][None], spk[r].view(1, 1), seed_frames=CFG["seed_frames"])
            for k, v in got[r].items():
                assert v.shape == alone[k].shape[1:] and v.shape[0] == t
                err = float((v - alone[k][0]).abs().max())
                print(f"{kind} {precision} recording {r} {k}: max|ragged - B=1| = {err:.3e}, bit-equal: {torch.equal(v, alone[k][0])}")
                assert err < 1e-4, (r, k, err)
            e6 = float(np.abs(got[r]["motion"].reshape(t, -1).cpu().numpy() - g[f"{kind}_{r}_motion"]).max())
            ea = float(np.abs(got[r]["motion_axis_angle"].cpu().numpy() - g[f"{kind}_{r}_axis_angle"]).max())
            print(f"{kind} {precision} recording {r}: vs reference rot-6D {e6:.3e}, axis-angle {ea:.3e}")
            assert e6 < 2e-4 and ea < 1e-3, (r, e6, ea)


@pytest.mark.parametrize("kind", ["disco", "camn"])
def test_runner_captured_equals_eager(kind):
    audios, spk = ragged_inputs()
    model = product(kind, "f16x3", DEV)
    rs = RecordingSet.from_audio(audios, DEV)
    eager = LR.LstmRecordingRunner.for_set(model, rs, use_graph=False, seed_frames=CFG["seed_frames"])
    graph = LR.LstmRecordingRunner.for_set(model, rs, use_graph=True, seed_frames=CFG["seed_frames"])
    assert graph.graph is not None and graph.order == [2, 0, 1] and graph.frames == list(RAGGED_FRAMES)
    assert graph.padded_share == pytest.approx(1 - sum(RAGGED_FRAMES) / (3 * max(RAGGED_FRAMES)))
    want = [tuple(x.copy() for x in r) for r in eager(rs)]
    first = [tuple(x.copy() for x in r) for r in graph(rs)]
    second = graph()
    for r, t in enumerate(RAGGED_FRAMES):                                        # input order although the runner sorts
        assert want[r][0].shape == (t, CFG["pose_dims"]) and want[r][1].shape == (t, 165)
        for a, b, c in zip(want[r], first[r], second[r]):
            assert np.array_equal(a, b) and np.array_equal(b, c)
    # ... and each recording is what forward_ragged gives it
    with torch.no_grad():
        direct = model.forward_ragged([a.to(DEV) for a in audios], spk.to(DEV), seed_frames=CFG["seed_frames"])
    for r, t in enumerate(RAGGED_FRAMES):
        assert np.array_equal(direct[r]["motion"].reshape(t, -1).cpu().numpy(), want[r][0])
    # other audio of the same lengths through the same graph
    other = RecordingSet.from_audio([a.flip(0) * 0.5 for a in audios], DEV)
    want2 = [tuple(x.copy() for x in r) for r in eager(other)]
    got2 = graph(other)
    for r in range(3):
        assert not np.array_equal(want2[r][0], want[r][0])
        for a, b in zip(want2[r], got2[r]):
            assert np.array_equal(a, b)
    # new weights are seen by the next call
    sd = {k: (v * 0.9 if v.is_floating_point() and k.startswith("body_out") else v) for k, v in model.state_dict().items()}
    model.load_state_dict(sd)
    want3 = [tuple(x.copy() for x in r) for r in eager(rs)]
    got3 = graph(rs)
    for r in range(3):
        assert not np.array_equal(want3[r][0], want[r][0])
        for a, b in zip(want3[r], got3[r]):
            assert np.array_equal(a, b)


def test_runner_cuts_batches_and_keeps_input_order():
    """max_batch = 2: two batches (36 | 34 frames, then 28 alone) in one graph — the same results as one batch of three."""
    audios, _spk = ragged_inputs()
    model = product("disco", "f16x3", DEV)
    rs = RecordingSet.from_audio(audios, DEV)
    one = LR.LstmRecordingRunner.for_set(model, rs, use_graph=False, seed_frames=CFG["seed_frames"])
    two = LR.LstmRecordingRunner.for_set(model, rs, max_batch=2, seed_frames=CFG["seed_frames"])
    assert two.batches == [[2, 0], [1]] and one.batches == [[2, 0, 1]]
    a = [tuple(x.copy() for x in r) for r in one(rs)]
    b = two(rs)
    for r, t in enumerate(RAGGED_FRAMES):
        assert b[r][0].shape == (t, CFG["pose_dims"])
        assert float(np.abs(a[r][0] - b[r][0]).max()) < 1e-4 and float(np.abs(a[r][1] - b[r][1]).max()) < 1e-3


def _write_wav(path, x):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes(x.astype("<i2").tobytes())


def test_generate_folder_lstm(tmp_path):
    audios, _spk = ragged_inputs()
    src, dst = tmp_path / "audio", tmp_path / "motion"
    src.mkdir()
    names = ["b_second", "a_first", "c_third"]                                   # sorted order differs from this one
    pcm = [np.clip(np.round(a.numpy() * 32768.0), -32768, 32767).astype(np.int16) for a in audios]
    for n, x in zip(names, pcm):
        _write_wav(src / f"{n}.wav", x)
    (src / "notes.txt").write_text("not audio")
    model = product("camn", "f16x3", DEV)
    written = LR.generate_folder_lstm(model, str(src), str(dst))
    by_name = dict(zip(names, range(3)))
    assert written == {f"{n}_output.npz": RAGGED_FRAMES[by_name[n]] for n in names}
    order = sorted(names)
    rs = RecordingSet.from_audio([torch.from_numpy(pcm[by_name[n]]) for n in order], DEV)
    assert rs.audio.dtype == torch.int16
    runner = LR.LstmRecordingRunner.for_set(model, rs, seed_frames=CFG["seed_frames"])
    for n, (_motion, aa) in zip(order, runner(rs)):
        rec = motion_io.beat_format_load(str(dst / f"{n}_output.npz"))
        t = RAGGED_FRAMES[by_name[n]]
        assert rec["poses"].shape == (2 * t, 165) and rec["trans"].shape == (2 * t, 3) and rec["expressions"].shape == (2 * t, 100)
        assert np.array_equal(rec["poses"], motion_io.time_upsample_numpy(aa, 2))
    # a runner handed in is reused (its graph replays)
    again = LR.generate_folder_lstm(model, str(src), str(tmp_path / "again"), runner=runner)
    assert again == written
    for n in names:
        assert np.array_equal(np.load(str(dst / f"{n}_output.npz"))["poses"], np.load(str(tmp_path / "again" / f"{n}_output.npz"))["poses"])
