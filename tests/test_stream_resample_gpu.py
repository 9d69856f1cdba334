"""The streaming resampler on the MI355X (emage_stream_push_resample, `StreamBatch(audio_inputs=...)`):
* the op against the OFFLINE kernel, bit for bit: five rates, s16 mono / stereo, f32 mono, s24 stereo, s32 six-channel, recordings of one
  frame to three output tiles, cut four ways, two slots of different formats per launch, a ring far shorter than the recording;
* the same outputs against the float64 restatement within the fp32 bound of the offline kernel's tests (tests/audio_common.py);
* idle slots behind canaries, every kind of bad row and bad argument, reproducibility, a slot reused at another rate;
* sessions of mixed formats against a 16 kHz batch fed `ops.audio_resample` of each whole recording: every emitted array and code equal,
  eager and captured; the reference's goldens through the new path; a window completed only by the outputs `end()` releases."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import audio_common
import common
import fake_stream_resample_ops as fk
import stream_common as sc
import stream_resample_common as rc
from pantomatrix_amd import _lib, audio, ops, streaming, synthetic
from pantomatrix_amd._lib import EmageKernelError
from pantomatrix_amd.audio import AudioInput, available, out_length

pytestmark = pytest.mark.gpu
DEV = "cuda"
RATES = [48000, 44100, 8000, 22050, 11025]
EXTRA = {22050: AudioInput(22050, 2, "s24"), 48000: AudioInput(48000, 6, "s32")}      # one s24 stereo and one s32 six-channel case


def inputs_of(rate):
    return (AudioInput(rate, 1, "s16"), AudioInput(rate, 2, "s16"), AudioInput(rate, 1, "f32")) + ((EXTRA[rate],) if rate in EXTRA else ())


def offline(pcm, inp):
    """`ops.audio_resample` over the whole recording: the samples the stream has to reproduce."""
    return ops.audio_resample(torch.from_numpy(np.ascontiguousarray(pcm)).to(DEV).unsqueeze(0), inp.channels, inp.rate)[0].cpu().numpy()


@functools.lru_cache(maxsize=None)
def streamed(rate):
    """Every (format, length, chunking) of one rate through the op, two formats per launch sequence in slots 0 and 1 -> [(input, n, chunking
    name, streamed samples, offline samples, frames)].  Computed once per rate, read-only; `run_plan` checks after every launch that exactly
    the outputs that became final were written."""
    inputs = inputs_of(rate)
    up, down = audio.rate_ratio(rate, 16000)
    rpp = int(ops.stream_formats(inputs)[0][0, 5])
    out = []
    for n in (rc.hi_frames(rate), 1, 37, 4411):
        pcm = [rc.clip(inp, n, seed=rate + 7 * i + n) for i, inp in enumerate(inputs)]
        want = [offline(p, inp) for p, inp in zip(pcm, inputs)]
        cuts, seen = [], set()
        for name, chunks in rc.plans(n, rpp, up, down).items():          # short recordings: several chunkings are the same list
            if tuple(chunks) not in seen:
                seen.add(tuple(chunks))
                cuts.append((name, chunks))
        for name, chunks in cuts:
            for lo in range(0, len(inputs), 2):                          # formats lo and lo + 1 side by side (an odd one out: beside an idle slot)
                pair = list(range(lo, min(lo + 2, len(inputs))))
                h = rc.Harness(inputs, [lo, (lo + 1) % len(inputs)], ring_len=rc.ring_for([chunks], up, down), dev=DEV)
                rc.run_plan(h, {k: pcm[i] for k, i in enumerate(pair)}, {k: chunks for k in range(len(pair))})
                assert all(rc.canaries_intact(w) for w in (h.ring_whole, h.hist_whole, h.taps_whole)) and rc.canaries_intact(h.staged_whole, 0xA5)
                # the ring is far shorter than a long recording cut into chunks: its writes wrap inside chunks, again and again
                assert len(chunks) == 1 or n < 100 or h.ring_len < len(want[lo])
                out += [(inputs[i], n, name, h.result(k), want[i], pcm[i]) for k, i in enumerate(pair)]
    return out


# ---- 1, 2: the op against the offline kernel and against float64 ----------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_streamed_samples_equal_the_offline_kernel_bit_for_bit(rate):
    cases = streamed(rate)
    assert {c[2] for c in cases if c[1] > 4000} == {"frame by frame, then 997", "shorter than rpp", "one chunk", "one output tile"}
    assert {c[0] for c in cases} == set(inputs_of(rate)) and {c[1] for c in cases} == {rc.hi_frames(rate), 1, 37, 4411}
    for inp, n, name, got, want, _pcm in cases:
        assert got.shape == want.shape == (out_length(n, *audio.rate_ratio(rate, 16000)),)
        assert torch.equal(torch.from_numpy(got), torch.from_numpy(want)), (inp, n, name, int((got != want).sum()))


@functools.lru_cache(maxsize=None)
def reference(rate, inp, n):
    pcm = rc.clip(inp, n, seed=rate + 7 * inputs_of(rate).index(inp) + n)
    return audio_common.reference_and_bound(rc.exact_mono(pcm, inp), *audio.rate_ratio(rate, 16000))


@pytest.mark.parametrize("rate", RATES)
def test_streamed_samples_match_float64_within_the_fp32_bound(rate):
    """The yardstick of the offline kernel's tests (audio_common.reference_and_bound), for the formats whose mono signal is exact in float64."""
    checked = 0
    for inp, n, name, got, _want, _pcm in streamed(rate):
        if inp.fmt == "s24" or inp.fmt == "s32":
            continue
        ref, bound = reference(rate, inp, n)
        err = np.abs(got.astype(np.float64) - ref)
        worst = int(np.argmax(err - bound))
        if name == "one chunk":
            print(f"{inp} n={n}: max|err| {err.max():.3e}, closest at m={worst}: {err[worst]:.3e} vs {bound[worst]:.3e}")
        assert err.shape == bound.shape and (err <= bound).all(), (inp, n, name, worst, float(err[worst]), float(bound[worst]))
        checked += 1
    assert checked >= 3 * 4 * 2


# ---- 3: canaries and refusals -----------------------------------------------------------------------------------------------------------------
INPUTS = (AudioInput(44100, 2, "s16"), AudioInput(48000, 1, "f32"), AudioInput(8000, 1, "s16"))


def three_slot_run():
    """Slots 0 and 2 stream (44.1 kHz stereo s16, 8 kHz mono s16); slot 1 never has a row."""
    h = rc.Harness(INPUTS, [0, 1, 2], ring_len=211, dev=DEV)
    pcm = {0: rc.clip(INPUTS[0], 1500, seed=1), 2: rc.clip(INPUTS[2], 700, seed=2)}
    rc.run_plan(h, pcm, {0: [1, 54, 400, 3, 500, 542], 2: [100] * 7})
    return h, pcm


def test_idle_slots_canaries_and_reproducibility():
    h, pcm = three_slot_run()
    assert bool((h.ring[1] == rc.CANARY).all()) and bool((h.history[1] == rc.CANARY).all()), "a slot with empty rows keeps its ring and both history sides"
    assert all(rc.canaries_intact(w) for w in (h.ring_whole, h.hist_whole, h.taps_whole)) and rc.canaries_intact(h.staged_whole, 0xA5)
    for k in (0, 2):
        assert np.array_equal(h.result(k), offline(pcm[k], INPUTS[k]))
    h2, _ = three_slot_run()                                                       # the same launches again: the same bits everywhere
    assert torch.equal(h.ring_whole, h2.ring_whole) and torch.equal(h.hist_whole, h2.hist_whole)
    assert all(np.array_equal(h.result(k), h2.result(k)) for k in (0, 2))


def test_bad_rows_set_bit_16_and_write_nothing():
    h, _ = three_slot_run()
    h.reopen(0, 0), h.reopen(2, 2)
    pcm = rc.clip(INPUTS[0], 600, seed=3)
    rows, host, used = h.rows({0: (pcm, False)})
    good = ops.stream_resample_table(rows, formats=h.desc, ring_len=h.ring_len, staged_bytes=h.staged.numel(), hist_len=h.hist_len)
    h.staged[:used].copy_(torch.from_numpy(host[:used]))
    before = (h.ring_whole.clone(), h.hist_whole.clone())
    bad_rows = {"source outside the staged buffer": (fk.SRC16, h.staged.numel() // 16 - 1), "count beyond the ring": (fk.OUT_COUNT, h.ring_len + 1),
                "format outside the descriptors": (fk.FORMAT, len(INPUTS)), "output position outside the ring": (fk.OUT_POS, h.ring_len),
                "negative format": (fk.FORMAT, -1), "an output that reads beyond the staged frames": (fk.OUT_COUNT, int(good[0, fk.OUT_COUNT]) + 1),
                "history longer than the buffer": (fk.HIST_VALID, h.hist_len + 1), "a third history side": (fk.HIST_SIDE, 2),
                "phase outside [0, up)": (fk.R0, 160), "negative kmax": (fk.KMAX0, -1), "negative frames": (fk.FRAMES, -5)}
    for what, (word, value) in bad_rows.items():
        raw = good.copy()
        raw[0, word] = value
        h.status.zero_()
        ops.stream_push_resample(h.staged, torch.from_numpy(raw).to(DEV), h.desc, h.taps, h.ring, h.history, h.status)
        assert int(h.status) == ops.STREAM_BAD_RESAMPLE == 16, what
        assert torch.equal(h.ring_whole, before[0]) and torch.equal(h.hist_whole, before[1]), what
    h.status.fill_(1)                                                              # the bit is ORed in: what the word held stays
    raw = good.copy()
    raw[0, fk.FORMAT] = 7
    ops.stream_push_resample(h.staged, torch.from_numpy(raw).to(DEV), h.desc, h.taps, h.ring, h.history, h.status)
    assert int(h.status) == 17
    h.status.zero_()
    ops.stream_push_resample(h.staged, torch.from_numpy(good).to(DEV), h.desc, h.taps, h.ring, h.history, h.status)      # the row as built: runs
    assert int(h.status) == 0 and not torch.equal(h.ring_whole, before[0]) and not torch.equal(h.hist_whole, before[1])
    assert all(rc.canaries_intact(w) for w in (h.ring_whole, h.hist_whole))


def test_bad_arguments_are_refused_before_any_launch():
    h, _ = three_slot_run()
    before = (h.ring_whole.clone(), h.hist_whole.clone())
    tab = torch.zeros(3, ops.STREAM_RS_WORDS, dtype=torch.int32, device=DEV)
    lib = _lib.load()
    desc = h.desc.reshape(-1).tolist()

    def call(staged=h.staged, staged_bytes=None, table=tab, slots=3, words=desc, n_formats=3, taps=h.taps, taps_floats=None, ring=h.ring,
             ring_len=h.ring_len, history=h.history, hist_len=h.hist_len, status=h.status):
        ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
        arr = (ctypes.c_int * len(words))(*words)
        return lib.emage_stream_push_resample(ptr(staged), h.staged.numel() if staged_bytes is None else staged_bytes, ptr(table), slots, arr, n_formats,
                                              ptr(taps), h.taps.numel() if taps_floats is None else taps_floats, ptr(ring), ring_len, ptr(history),
                                              hist_len, ptr(status), torch.cuda.current_stream().cuda_stream)
    assert call() == 0
    wrong = lambda word, value: desc[:word] + [value] + desc[word + 1:]
    refused = [call(staged=None), call(table=None), call(ring=None), call(history=None), call(status=None), call(taps=None),
               call(staged=h.staged.data_ptr() + 8), call(taps=h.taps.data_ptr() + 4), call(ring=h.ring.data_ptr() + 2), call(table=tab.data_ptr() + 1),
               call(slots=0), call(staged_bytes=0), call(ring_len=0), call(ring_len=1 << 31), call(hist_len=0), call(hist_len=54), call(n_formats=0),
               call(n_formats=9), call(taps_floats=100),
               call(words=wrong(0, 4)), call(words=wrong(1, 9)), call(words=wrong(2, 0)), call(words=wrong(3, 1 << 17)), call(words=wrong(4, 4400)),
               call(words=wrong(5, 55)), call(words=wrong(6, 56)), call(words=wrong(7, 2)), call(words=wrong(7, -4))]
    assert refused == [-1] * len(refused)                                          # EMAGE_EINVAL
    with pytest.raises(EmageKernelError):
        ops.stream_push_resample(h.staged[1:], tab, h.desc, h.taps, h.ring, h.history, h.status)              # a staged buffer off its 16-byte boundary
    with pytest.raises(EmageKernelError):
        ops.stream_push_resample(h.staged, tab, h.desc, h.taps, h.ring, h.history[:, :, :10].contiguous(), h.status)      # a history shorter than rpp - 1
    torch.cuda.synchronize()
    assert torch.equal(h.ring_whole, before[0]) and torch.equal(h.hist_whole, before[1]) and int(h.status) == 0


# ---- 4: a slot reused at another rate ---------------------------------------------------------------------------------------------------------
def test_a_reused_slot_sees_no_stale_history():
    h = rc.Harness(INPUTS, [0], ring_len=401, dev=DEV)
    first = rc.clip(INPUTS[0], 2000, seed=4, which=2)                              # full-scale frames: what a stale history would leak
    rc.run_plan(h, {0: first}, {0: [700, 700, 600]})
    assert np.array_equal(h.result(0), offline(first, INPUTS[0])) and bool((h.history[0] != rc.CANARY).all())
    h.reopen(0, 2)                                                                 # an 8 kHz session in the same slot, the buffers as they are
    second = rc.clip(INPUTS[2], 300, seed=5)
    rc.run_plan(h, {0: second}, {0: [7, 13, 1, 100, 179]})
    assert np.array_equal(h.result(0), offline(second, INPUTS[2]))


# ---- 5 - 7: sessions ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models():
    return {p: common.product_models(precision=p, device=DEV) for p in ("fp32", "f16x3")}


def make_batch(models, precision="f16x3", use_graph=False, **kw):
    return streaming.StreamBatch(*models[precision], slots=3, max_seconds=11, use_graph=use_graph, **kw)


def recording(inp, frames, seed):
    return rc.clip(inp, inp.frames_for(synthetic.samples_for_frames(frames)), seed)


@pytest.fixture(scope="module")
def plain(models):
    """An ordinary eager 16 kHz f32 batch, shared."""
    return make_batch(models)


@pytest.mark.parametrize("use_graph", [False, True])
def test_mixed_format_sessions_equal_the_16_khz_batch_bit_for_bit(models, plain, use_graph):
    """310 frames of 44.1 kHz stereo s16 and 70 of 8 kHz mono s16 open together, 129 of 48 kHz mono f32 a tick later; the 8 kHz session closes
    after one window while the others run on."""
    frames = (310, 129, 70)
    pcm = [recording(inp, f, seed=20 + i) for i, (inp, f) in enumerate(zip(INPUTS, frames))]
    opens, chunks = (0, 1, 0), (4099, 7001, 1237)
    mixed = make_batch(models, use_graph=use_graph, audio_inputs=INPUTS)
    assert (mixed.graph is not None) == use_graph
    got, slots = rc.run_sessions(mixed, [(opens[i], pcm[i], INPUTS[i], chunks[i]) for i in range(3)])
    want, slots_b = rc.run_sessions(plain, [(opens[i], offline(pcm[i], INPUTS[i]), None, 5000) for i in range(3)])
    assert slots == slots_b == [0, 2, 1]
    for i, inp in enumerate(INPUTS):
        rounds, t = streaming.tail_of(out_length(len(pcm[i]), *audio.rate_ratio(inp.rate, 16000)))
        assert got[i][0].shape[0] == 60 * rounds + t == frames[i]
        assert rc.same(got[i], want[i]), (use_graph, inp)


@pytest.fixture(scope="module")
def decode_only(models):
    """The five-session scenario of the stream tests, unchanged, through batches that take 16 kHz mono f32 by the new path."""
    return {p: sc.scenario(make_batch(models, p, audio_inputs=(AudioInput(16000, 1, "f32"),)), sc.waves()) for p in models}


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", list("ABCDE"))
def test_goldens_through_the_new_path(decode_only, golden_dir, precision, name):
    sc.check_against_golden(name, decode_only[precision][name], golden_dir, f"{precision} audio_inputs")


def test_the_outputs_held_back_can_complete_a_window_at_the_end(models, plain):
    up, down = 160, 441
    need = streaming.window_need(0)
    n = next(n for n in range(need * down // up - 2, need * down // up + 3) if out_length(n, up, down) >= need)
    assert available(n, up, down) < need <= out_length(n, up, down)                # the premise: the window is complete only once the input has ended
    pcm = rc.clip(INPUTS[0], n, seed=9)
    want = sc.run_alone(plain, offline(pcm, INPUTS[0]))
    mixed = make_batch(models, audio_inputs=INPUTS)
    s = mixed.open()
    s.push(pcm)
    assert not s.ready and mixed.step() == {}
    with pytest.raises(RuntimeError, match="still pending"):
        s.close()
    assert s.ended and not s.closed and s.ready
    out = mixed.step()
    assert rc.same(sc.joined([out[s], s.close()]), want) and s.windows == 1
    s = mixed.open()                                                               # the other order: end(), step() until nothing runs, close()
    s.push(pcm[:50000]), s.push(pcm[50000:])
    s.end()
    pieces = []
    while True:
        out = mixed.step()
        if not out:
            break
        pieces.append(out[s])
    pieces.append(s.close())
    assert len(pieces) == 2 and rc.same(sc.joined(pieces), want)
