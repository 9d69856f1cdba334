"""The streaming resampler without a device (pantomatrix_amd/streaming.py with `audio_inputs=`, over tests/fake_stream_resample_ops.py):
* rule 4 — `available(n)` outputs of a prefix of n frames are final, and no more than those;
* the second table's builder: relative words that fit int32 an hour into a session, every kind of invalid row refused;
* the host protocol: push layouts per format, `end()`, declared inputs, the ring in 16 kHz units, the counters, the history side;
* a default batch never calls the new op; a mixed-format batch equals the 16 kHz batch fed the whole recordings resampled."""
import numpy as np
import pytest
import torch

import audio_common
import common
import fake_ops
import fake_stream_resample_ops as fk
import stream_common as sc
import stream_resample_common as rc
from pantomatrix_amd import audio, ops, streaming, synthetic
from pantomatrix_amd.audio import AudioInput, available, out_length

RATES = [48000, 44100, 8000, 22050, 11025, 24000, 32000, 96000]
INPUTS = (AudioInput(44100, 2, "s16"), AudioInput(48000, 1, "f32"), AudioInput(8000, 1, "s16"))


# ---- rule 4 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_available_outputs_are_final_and_no_others(rate):
    up, down = audio.rate_ratio(rate, 16000)
    half = audio.half_length(up, down)
    rpp = -(-(2 * half + 1) // up)
    total = 6 * rpp + 41
    x = np.random.default_rng(rate).standard_normal(total)
    y = audio.resample_host(x, up, down)
    for n in sorted({1, 2, rpp - 1, rpp, rpp + 1, 2 * rpp + 3, total // 2, total - 1, total}):
        a = available(n, up, down)
        assert 0 <= a <= out_length(n, up, down)
        assert np.array_equal(audio.resample_host(x[:n], up, down)[:a], y[:a]), (n, a)       # a prefix's first a outputs: those of the whole
        assert (a * down + half) // up >= n                                                   # output a reads frame n or a later one, through a real tap
        assert 0 <= a * down + half - ((a * down + half) // up) * up <= 2 * half
        assert a == 0 or ((a - 1) * down + half) // up < n
    assert available(0, up, down) == 0 and available(total, 1, 1) == total                  # no filter, nothing held back


# ---- the table builder -------------------------------------------------------------------------------------------------------------------------
GEOMETRY = dict(ring_len=82234, staged_bytes=1 << 20)


def test_table_words_are_relative_and_fit_int32_an_hour_in():
    desc, _taps, hist_len = ops.stream_formats(INPUTS)
    up, down, half = 160, 441, 4410
    before = 44100 * 3600 + 17
    m0, frames = available(before, up, down), 4411
    count = available(before + frames, up, down) - m0
    assert m0 * down > 2 ** 31 and before * 4 > 2 ** 29
    tab = ops.stream_resample_table([None, dict(frames=frames, src=32, format=0, frames_before=before, outputs_before=m0, out_count=count, hist_side=1)],
                                    formats=desc, hist_len=hist_len, **GEOMETRY)
    assert tab.dtype == np.int32 and tab.shape == (2, ops.STREAM_RS_WORDS) and not tab[0].any()
    kmax0, r0 = (m0 * down + half) // up - before, (m0 * down + half) % up
    assert tab[1].tolist()[:10] == [frames, 2, 0, 0, count, m0 % 82234, kmax0, r0, hist_len, 1]
    assert 0 <= kmax0 <= 3 and kmax0 + ((count - 1) * down + r0) // up < frames <= kmax0 + (count * down + r0) // up
    # the flush: no frames, the outputs up to ceil(n up / down)
    total = before + frames
    rest = out_length(total, up, down) - (m0 + count)
    tab = ops.stream_resample_table([dict(format=0, final=1, frames_before=total, outputs_before=m0 + count, out_count=rest, hist_side=0)],
                                    formats=desc, hist_len=hist_len, **GEOMETRY)
    assert 10 <= rest <= 21 and tab[0].tolist()[:5] == [0, 0, 0, 1, rest]


def test_table_refuses_every_kind_of_invalid_row():
    desc, _taps, hist_len = ops.stream_formats(INPUTS)
    up, down = 160, 441
    before = 1000
    m0 = available(before, up, down)
    good = dict(frames=441, src=0, format=0, frames_before=before, outputs_before=m0, out_count=available(before + 441, up, down) - m0, hist_side=0)
    build = lambda rows, **kw: ops.stream_resample_table(rows, formats=desc, hist_len=hist_len, **{**GEOMETRY, **kw})
    assert build([good])[0, 0] == 441
    for change in (dict(format=3), dict(format=-1), dict(frames=-1), dict(src=8), dict(src=-16), dict(src=(1 << 20) - 16), dict(hist_side=2),
                   dict(out_count=good["out_count"] + 1),                   # an output that reads beyond the staged frames, no final flag
                   dict(out_count=good["out_count"] + 30, final=1),         # beyond ceil(n up / down)
                   dict(outputs_before=m0 - 1),                             # an output that was due in an earlier launch
                   dict(frames_before=-1), dict(out_count=-1), dict(push_count=3)):
        with pytest.raises(ValueError):
            build([{**good, **change}])
    with pytest.raises(ValueError):
        build([dict(good, out_count=9)], ring_len=8)                        # more outputs than the ring holds
    with pytest.raises(ValueError):
        build([good, dict(good, src=16)])                                   # two chunks overlap in the staged buffer
    assert not build([dict(frames=0, out_count=0, format=99)]).any()        # a row with nothing to do is empty, whatever else it says


def test_declared_formats_are_checked():
    desc, taps, hist_len = ops.stream_formats(INPUTS + (AudioInput(16000, 1, "f32"), AudioInput(96000, 6, "s32"), AudioInput(22050, 2, "s24")))
    assert desc.shape == (6, ops.STREAM_FORMAT_WORDS) and hist_len == 120                      # 96 kHz: rpp = 121
    assert desc[0].tolist() == [0, 2, 160, 441, 4410, 56, 57, 0] and desc[3].tolist() == [3, 1, 1, 1, 0, 1, 0, 0]
    for i in (0, 1, 2, 4, 5):
        _pcm, _ch, up, down, half, rpp, pitch, off = desc[i].tolist()
        want = audio.pack_taps(audio.resample_filter(up, down), up)
        assert off % 4 == 0 and want.shape == (up, pitch) and np.array_equal(taps[off:off + up * pitch].reshape(up, pitch), want)
    assert ops.stream_formats((AudioInput(16000, 2, "s16"),))[2] == 1
    for bad in ((), INPUTS * 3, (AudioInput(44100, 9, "s16"),), (AudioInput(44100, 0, "s16"),), (AudioInput(44101, 1, "s16"),), (AudioInput(0, 1, "s16"),),
                ((44100, 1, "s16"),)):
        with pytest.raises(ValueError):
            ops.stream_formats(bad)


# ---- the op's stand-in against the whole-clip arithmetic and float64 ---------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [44100, 8000, 16000])
def test_stand_in_streams_equal_the_whole_clip(rate):
    inputs = (AudioInput(rate, 1, "s16"), AudioInput(rate, 2, "f32"))
    up, down = audio.rate_ratio(rate, 16000)
    n = 3 * rc.TILE // 8 * down // up + 1
    pcm = {0: rc.clip(inputs[0], n, seed=rate), 1: rc.clip(inputs[1], n + 5, seed=rate + 1)}
    rpp = int(ops.stream_formats(inputs)[0][0, 5])
    for names in (("frame by frame, then 997", "shorter than rpp"), ("one chunk", "one output tile")):
        plan = {k: rc.plans(len(pcm[k]), rpp, up, down)[nm] for k, nm in zip(pcm, names)}
        h = rc.Harness(inputs, [0, 1], ring_len=rc.ring_for(plan.values(), up, down), dev="cpu", op=fk.stream_push_resample)
        rc.run_plan(h, pcm, plan)
        for k in pcm:
            assert np.array_equal(h.result(k), fk.resample_whole(rc.as_bytes(pcm[k]), inputs[k])), (names, k)
        assert all(rc.canaries_intact(w) for w in (h.ring_whole, h.hist_whole, h.taps_whole)) and rc.canaries_intact(h.staged_whole, 0xA5)
    if rate != 16000:
        for k in pcm:
            ref, bound = audio_common.reference_and_bound(rc.exact_mono(pcm[k], inputs[k]), up, down)
            assert (np.abs(h.result(k).astype(np.float64) - ref) <= bound).all()


# ---- the host protocol -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models():
    return common.product_models(precision="fp32")


def make_batch(models, **kw):
    with fk.installed(), torch.no_grad():
        return streaming.StreamBatch(*models, slots=3, max_seconds=11, use_graph=False, **kw)


@pytest.fixture(scope="module")
def batch(models):
    sb = make_batch(models, audio_inputs=INPUTS)
    assert sb.ring_len == 82234 and sb.hist_len == 60 and sb.staged.dtype == torch.uint8
    # staging is sized from the formats: 48 kHz mono f32 has the most bytes per 16 kHz sample (12; 44.1 kHz stereo s16 has 11.025)
    assert sb.staged.numel() == 3 * (-(-((82234 * 3 + 30) // 1 + 2) * 4 // 16) * 16)
    return sb


def quiet(batch, monkeypatch):
    """The forward stubbed out: the push launch (the stand-in) and the host's bookkeeping remain."""
    monkeypatch.setattr(batch, "_tick", batch._launch_push)
    monkeypatch.setattr(batch, "_finish", lambda s, rounds, t: None)


def test_push_layouts_and_end(batch, monkeypatch):
    quiet(batch, monkeypatch)
    with fk.installed():
        with pytest.raises(ValueError):
            batch.open(audio_input=AudioInput(44100, 1, "s16"))                    # not declared
        a, b, c = batch.open(), batch.open(audio_input=INPUTS[1]), batch.open(audio_input=AudioInput(8000, 1, "s16"))
        assert (a.fmt, b.fmt, c.fmt) == (0, 1, 2)
        for bad in (np.zeros(8, np.int16), np.zeros((8, 1), np.int16), np.zeros((8, 2), np.float32), np.zeros((8, 2), np.int32), np.zeros((2, 8), np.int16)):
            with pytest.raises(ValueError):
                a.push(bad)
        for bad in (np.zeros(8, np.int16), np.zeros((8, 2), np.float32), np.zeros(8, np.float64)):
            with pytest.raises(ValueError):
                b.push(bad)
        a.push(np.zeros((0, 2), np.int16)), b.push(np.zeros(7, np.float32)), b.push(torch.zeros(3, 1)), c.push(np.zeros((5, 1), np.int16)), c.push(np.zeros(6, np.int16))
        assert (a.frames_in, b.frames_in, c.frames_in) == (0, 10, 11) and (a.pushed, b.pushed) == (0, 0) and c.pushed == available(11, 2, 1) == 2
        a.push(np.zeros((100, 2), np.int16))
        assert a.frames_in == 100 and a.pushed == available(100, 160, 441) == 27
        c.end(), c.end()
        assert c.ended and c.pushed == out_length(11, 2, 1) == 22
        with pytest.raises(RuntimeError, match="ended"):
            c.push(np.zeros(1, np.int16))
        for s in (a, b, c):
            s.close()
        assert a.pushed == out_length(100, 160, 441) == 37 and a.closed
    plain = make_batch((batch.model, batch.vq))
    with fk.installed(), pytest.raises(ValueError):
        plain.open(audio_input=INPUTS[0])                                          # a batch without declared inputs


def test_s24_s32_and_many_channel_layouts(models, monkeypatch):
    sb = make_batch(models, audio_inputs=(AudioInput(22050, 2, "s24"), AudioInput(96000, 6, "s32")))
    quiet(sb, monkeypatch)
    with fk.installed():
        a, b = sb.open(), sb.open(audio_input=AudioInput(96000, 6, "s32"))
        a.push(np.zeros((9, 6), np.uint8)), b.push(np.zeros((9, 6), np.int32))
        for s, bad in ((a, np.zeros((9, 2), np.uint8)), (a, np.zeros((9, 6), np.int8)), (b, np.zeros((9, 6), np.float32)), (b, np.zeros((9, 2), np.int32))):
            with pytest.raises(ValueError):
                s.push(bad)
        assert a.frames_in == b.frames_in == 9
        a.close(), b.close()
    with fk.installed(), pytest.raises(ValueError):
        streaming.StreamBatch(*models, slots=1, max_seconds=4, use_graph=False, audio_inputs=(AudioInput(44101, 1, "s16"),))


def test_the_ring_is_counted_in_16_khz_samples(batch, monkeypatch):
    quiet(batch, monkeypatch)
    with fk.installed():
        s = batch.open(audio_input=INPUTS[2])                                      # 8 kHz: two outputs a frame
        s.push(np.zeros(41117, np.int16))                                          # 82 234 samples once ended: the ring, exactly
        assert s.pushed == 82234 - 20
        with pytest.raises(ValueError, match="do not fit"):
            s.push(np.zeros(1, np.int16))
        s._staged, s.pushed, s.frames_in = [], 0, 0                                # drop the backlog: nothing of it reached the device
        s.close()
        s = batch.open(audio_input=INPUTS[2])
        with pytest.raises(ValueError, match="max_seconds"):
            s.push(np.zeros(11 * 8000 + 1, np.int16))
        s.close()


def test_history_side_flips_with_each_push_of_its_slot_only(batch, monkeypatch):
    quiet(batch, monkeypatch)
    words = []

    def flush():
        rows, staged = batch._rows([])
        batch._upload(rows, staged)
        batch._launch_push()
        words.append(batch.rs_table_host.clone().numpy())
    with fk.installed():
        sides0 = list(batch.hist_side)
        a, b = batch.open(), batch.open(audio_input=INPUTS[2])
        a.push(np.ones((500, 2), np.int16)), b.push(np.ones(300, np.int16))
        flush()
        a.push(np.ones((3, 2), np.int16))                                          # no output becomes final: the history still moves
        flush()
        flush()                                                                    # nothing staged: empty rows, no flip
        a.push(np.ones((40, 2), np.int16)), b.push(np.ones(1, np.int16))
        flush()
        b.end()
        flush()                                                                    # b's flush alone: no frames, no flip
        t = np.stack(words)
        assert t[:, 0, fk.HIST_SIDE].tolist()[:2] == [sides0[0], sides0[0] ^ 1] and t[3, 0, fk.HIST_SIDE] == sides0[0] and batch.hist_side[0] == sides0[0] ^ 1
        assert t[0, 1, fk.HIST_SIDE] == sides0[1] and t[3, 1, fk.HIST_SIDE] == sides0[1] ^ 1 and t[4, 1, fk.HIST_SIDE] == sides0[1] and batch.hist_side[1] == sides0[1]
        assert t[:, 0, fk.FRAMES].tolist() == [500, 3, 0, 40, 0] and t[1, 0, fk.OUT_COUNT] == available(503, 160, 441) - available(500, 160, 441)
        assert not t[2].any() and t[:, 0, fk.HIST_VALID].tolist() == [0, 60, 0, 60, 0] and t[3, 1, fk.HIST_VALID] == 60
        assert t[4, 1].tolist()[:5] == [0, 0, 2, 1, 602 - available(301, 2, 1)] and not t[4, 0].any()
        assert (a._sent, a._written, b._sent, b._written) == (543, available(543, 160, 441), 301, 602)
        a.close(), b.close()
        c = batch.open(audio_input=INPUTS[1])                                      # slot 0 again: the new session starts without history
        c.push(np.ones(700, np.float32))
        flush()
        assert c.slot == 0 and words[-1][0, fk.HIST_VALID] == 0 and words[-1][0, fk.KMAX0] == 30    # kmax of output 0 at 48 kHz: half / up
        c.close()


# ---- sessions ----------------------------------------------------------------------------------------------------------------------------------
def recording(inp, frames, seed):
    """Frames of `inp` whose 16 kHz length just reaches the samples of `frames` video frames."""
    return rc.clip(inp, inp.frames_for(synthetic.samples_for_frames(frames)), seed)


def as_16k(pcm, inp):
    return fk.resample_whole(rc.as_bytes(pcm), inp)


def test_a_default_batch_never_calls_the_new_op(models):
    sb = make_batch(models)
    with fk.installed(), torch.no_grad():
        fake_ops.CALLS.clear()
        s = sb.open()
        s.push(np.zeros(synthetic.samples_for_frames(40), np.float32))
        s.end()
        assert s.pushed == s.frames_in == synthetic.samples_for_frames(40)
        assert s.close().poses.shape == (40, 165)
        calls = set(fake_ops.CALLS)
    assert "stream_push" in calls and "stream_push_resample" not in calls and not hasattr(sb, "history")


def test_mixed_formats_equal_the_16_khz_batch_on_resampled_audio(batch, models):
    """129 frames of 44.1 kHz stereo s16 and 70 of 48 kHz mono f32 open together; the second closes after one window and 40 frames of 8 kHz
    mono s16 take its slot — against a 16 kHz f32 batch fed, in the same slots, each whole recording resampled in the same arithmetic."""
    pcm = [recording(INPUTS[0], 129, 1), recording(INPUTS[1], 70, 2), recording(INPUTS[2], 40, 3)]
    plain = make_batch(models)
    with fk.installed(), torch.no_grad():
        fake_ops.CALLS.clear()
        got, slots = rc.run_sessions(batch, [(0, pcm[0], INPUTS[0], 4099), (0, pcm[1], INPUTS[1], 7001), (2, pcm[2], INPUTS[2], 1237)])
        calls = set(fake_ops.CALLS)
        want, slots_b = rc.run_sessions(plain, [(0, as_16k(pcm[0], INPUTS[0]), None, 5000), (0, as_16k(pcm[1], INPUTS[1]), None, 5000),
                                                (2, as_16k(pcm[2], INPUTS[2]), None, 5000)])
    assert "stream_push_resample" in calls and "stream_push" not in calls
    assert slots == slots_b == [0, 1, 1]
    for i, (inp, frames) in enumerate(zip(INPUTS, (129, 70, 40))):
        rounds, t = streaming.tail_of(out_length(len(pcm[i]), *audio.rate_ratio(inp.rate, 16000)))
        assert got[i][0].shape[0] == 60 * rounds + t == frames and rc.same(got[i], want[i]), i


def test_the_outputs_held_back_can_complete_a_window_at_the_end(batch, models):
    up, down = 160, 441
    need = streaming.window_need(0)
    n = next(n for n in range(need * down // up - 2, need * down // up + 3) if out_length(n, up, down) >= need)
    assert available(n, up, down) < need <= out_length(n, up, down)                # the premise: the window is complete only once the input has ended
    pcm = rc.clip(INPUTS[0], n, seed=9)
    plain = make_batch(models)
    with fk.installed(), torch.no_grad():
        want = sc.run_alone(plain, as_16k(pcm, INPUTS[0]))
        s = batch.open()
        s.push(pcm)
        assert not s.ready and batch.step() == {}
        with pytest.raises(RuntimeError, match="still pending"):
            s.close()
        assert s.ended and not s.closed and s.ready and batch.sessions[s.slot] is s
        out = batch.step()
        got = sc.joined([out[s], s.close()])
        assert rc.same(got, want) and s.windows == 1
        s = batch.open()                                                           # the other order: end(), step() until nothing runs, close()
        s.push(pcm[:50000]), s.push(pcm[50000:])
        s.end()
        pieces = []
        while True:
            out = batch.step()
            if not out:
                break
            pieces.append(out[s])
        pieces.append(s.close())
        assert len(pieces) == 2 and rc.same(sc.joined(pieces), want)
