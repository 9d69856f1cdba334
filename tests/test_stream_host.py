"""The streaming batch without a device (pantomatrix_amd/streaming.py over the stand-ins of tests/fake_stream_ops.py):
* rule 1 — the windows a session runs, whatever the push chunking, are the reference's for the total it is closed at;
* rule 2 — the decode's radius, by perturbing one code: R_part for the poses, `lag` for everything;
* the five-session scenario against the REFERENCE's B = 1 goldens: codes identical, arrays within the project's 1e-3;
* the table builder and the stand-ins' ring arithmetic against numpy slicing."""
import numpy as np
import pytest
import torch

import common
import fake_ops
import fake_stream_ops
import stream_common as sc
from pantomatrix_amd import ops, streaming, synthetic
from test_recordings_host import reference_windows


@pytest.fixture(scope="module")
def models():
    return common.product_models(precision="fp32")


@pytest.fixture(scope="module")
def batch(models):
    """One eager 3-slot batch on the CPU models; max_seconds = 11 with max_push = 48 000 gives a ring of 82 234 samples, which the
    165 334 samples of the longest waveform wrap twice."""
    with fake_stream_ops.installed(), torch.no_grad():
        sb = streaming.StreamBatch(*models, slots=3, max_seconds=11, use_graph=False)
    assert sb.lag == 28 and sb.r_part == 7 and sb.seg_len == 116 and sb.ring_codes == 120 and sb.ring_len == 34134 + 20 * 5 + 48000
    return sb


# ---- rule 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [1000, 40000])
def test_windows_run_equal_the_reference_schedule(batch, chunk, monkeypatch):
    """The launches are stubbed out: this is the host's bookkeeping alone, one session after another in slot 0."""
    tails = []
    monkeypatch.setattr(batch, "_tick", lambda: None)
    monkeypatch.setattr(batch, "_finish", lambda s, rounds, t: tails.append((60 * rounds, t)))
    wave = np.zeros(synthetic.samples_for_frames(200), dtype=np.float32)
    with fake_stream_ops.installed():
        for n in range(0, len(wave), 997):
            s, ran = batch.open(), []
            for lo in range(0, n, chunk):
                s.push(wave[lo:min(lo + chunk, n)])
                while batch.step():
                    ran.append((60 * (s.windows - 1), 60 * (s.windows - 1) + 64, 60))
            del tails[:]
            s.close()
            if tails[0][1]:
                ran.append((tails[0][0], tails[0][0] + tails[0][1], tails[0][1]))
            total = n * 30 // 16000
            want = reference_windows(total) if total > 4 else []
            assert ran == want and s.emitted == sum(w[2] for w in want), (n, ran, want)


def test_a_window_waits_for_the_samples_of_rule_1(batch, monkeypatch):
    monkeypatch.setattr(batch, "_tick", lambda: None)
    monkeypatch.setattr(batch, "_finish", lambda s, rounds, t: None)
    with fake_stream_ops.installed():
        s = batch.open()
        s.push(np.zeros(64 * 533, dtype=np.float32))                   # the samples window 0 READS: 63 frames by M:345, a tail for the reference
        assert not s.ready and batch.step() == {}
        s.push(np.zeros(streaming.window_need(0) - 64 * 533 - 1, dtype=np.float32))
        assert not s.ready
        s.push(np.zeros(1, dtype=np.float32))
        assert s.ready and streaming.window_need(0) == 34134 and streaming.window_need(1) == 34134 + 32000
        with pytest.raises(RuntimeError):
            s.close()                                                   # a full window is pending
        assert list(batch.step()) == [s]
        s.close()


def test_a_push_that_does_not_fit_raises(batch, monkeypatch):
    monkeypatch.setattr(batch, "_finish", lambda s, rounds, t: None)
    with fake_stream_ops.installed():
        s = batch.open()
        s.push(np.zeros(batch.ring_len, dtype=np.float32))
        with pytest.raises(ValueError):
            s.push(np.zeros(1, dtype=np.float32))
        with pytest.raises(ValueError):
            s.push(np.zeros((2, 8), dtype=np.float32))
        with pytest.raises(ValueError):
            s.push(np.zeros(8, dtype=np.float64))
        others = [batch.open(), batch.open()]
        with pytest.raises(RuntimeError):
            batch.open()                                                # no slot is free
        s._staged, s.pushed = [], 0                                     # drop the backlog: nothing of it reached the device
        for x in [s] + others:
            x.close()


def test_cpu_weights_and_health_counter_raise():
    model, vq = common.product_models(precision="fp32")                 # its own models: the test moves their version stamp
    with pytest.raises(RuntimeError):
        streaming.StreamBatch(model, vq, slots=1)                       # on the CPU, like every runner
    with fake_stream_ops.installed(), torch.no_grad():
        sb = streaming.StreamBatch(model, vq, slots=1, max_seconds=4, use_graph=False)
        with pytest.raises(ValueError):
            sb.open(speaker_id=int(model.config.speaker_dims))
        with pytest.raises(ValueError):
            sb.open(seed=torch.zeros(4, 330))
        s = sb.open()
        with pytest.raises(ValueError):
            s.push(np.zeros(4 * 16000 + 1, dtype=np.float32))           # longer than max_seconds
        s.push(np.zeros(streaming.window_need(0), dtype=np.float32))
        sb.nonfinite += 2                                               # what the health counter holds behind non-finite logits (the stand-ins
        with pytest.raises(FloatingPointError):                         # refuse non-finite operands: the GPU test pushes NaN audio)
            sb.step()
        assert int(sb.nonfinite) == 0 and s.windows == 0
        w = dict(model.named_parameters())["face_out_proj.weight"]
        with torch.no_grad():
            w.mul_(1.0)                                                 # in place: the version stamp moves, the values do not
        with pytest.raises(RuntimeError, match="fixed for the life"):
            sb.step()


# ---- rule 2 ------------------------------------------------------------------------------------------------------------------------------
def _changed_frames(vq, frame=150, frames=310):
    g = torch.Generator().manual_seed(3)
    codes = {f"{p}_index": torch.randint(0, 256, (1, frames), generator=g) for p in sc.PARTS}
    ref = torch.zeros(1, 3)
    with fake_ops.installed(), torch.no_grad():
        base = vq.decode(**codes, get_global_motion=True, ref_trans=ref)
        aa, expr, vel = vq._decode_segments(**codes)
        assert torch.equal(aa.view(1, frames, 165), base["motion_axis_angle"]) and torch.equal(expr.view(1, frames, 100), base["expression"])
        other = {k: v.clone() for k, v in codes.items()}
        for v in other.values():
            v[0, frame] = (v[0, frame] + 1) % 256
        aa2, expr2, vel2 = vq._decode_segments(**other)
    rows = lambda a, b: set(torch.nonzero((a != b).reshape(frames, -1).any(dim=1)).flatten().tolist())
    return rows(aa, aa2), rows(expr, expr2) | rows(vel[:, 54:57], vel2[:, 54:57])


def test_one_code_reaches_the_radius_and_no_further(models, batch):
    poses, rest = _changed_frames(models[1])
    assert 143 in poses and 157 in poses and poses <= set(range(143, 158))
    assert (poses | rest) <= set(range(150 - batch.lag, 150 + batch.lag + 1))
    assert max(rest) > 157                                              # the translation path does reach beyond the poses' radius


def test_radius_of_the_three_layer_stacks():
    import pantomatrix_amd as pa
    from pantomatrix_amd import synthetic as syn
    _acfg, vqc, gc = common.cfg_dicts(vae_layer=3, global_layer=3)
    parts = {}
    for p in sc.PARTS:
        c = pa.EmageVQVAEConvConfig(**vqc[p])
        parts[p] = pa.EmageVQVAEConv(c)
        parts[p].load_state_dict(syn.vqvae_state(c, p, 0))
    g = pa.EmageVAEConv(pa.EmageVAEConvConfig(**gc))
    g.load_state_dict(syn.vae_state(pa.EmageVAEConvConfig(**gc), 0))
    vq = pa.EmageVQModel(face_model=parts["face"], upper_model=parts["upper"], hands_model=parts["hands"], lower_model=parts["lower"],
                         global_model=g).set_precision("fp32").eval()
    r_part, lag = streaming.decode_radius(vq)
    assert (r_part, lag) == (8, 8 + 5 + 12)
    poses, rest = _changed_frames(vq)
    assert 142 in poses and 158 in poses and poses <= set(range(142, 159))
    assert (poses | rest) <= set(range(150 - lag, 150 + lag + 1))


# ---- the scenario against the reference ----------------------------------------------------------------------------------------------------
def test_five_sessions_match_the_reference_goldens(batch, golden_dir):
    with fake_stream_ops.installed(), torch.no_grad():
        fake_ops.CALLS.clear()
        got = sc.scenario(batch, sc.waves())
        calls = list(fake_ops.CALLS)
    ticks = 1 + 1 + 3                                                   # A's five windows; B's, C's and D's run beside them
    assert calls.count("stream_windows") == ticks + 4 and calls.count("stream_commit") == ticks      # + one per tail (A, B, C, E)
    assert calls.count("stream_emit") == ticks + 5
    for name in "ABCDE":
        sc.check_against_golden(name, got[name], golden_dir, "host fp32")


# ---- the table builder and the rings -------------------------------------------------------------------------------------------------------
GEOMETRY = dict(ring_len=40000, staged_samples=3 * 5921, samples=64 * 533, ring_codes=120, seg_len=116, out_rows=60)


def test_stream_table_checks_what_it_builds():
    tab = ops.stream_table([dict(push_count=5921, push_src=0, audio_write=39999), None,
                            dict(ready=1, audio_read=39999, code_write=60, seg_read=4, seg_valid=116, emit_row=28, emit_count=60)], **GEOMETRY)
    assert tab.dtype == np.int32 and tab.shape == (3, ops.STREAM_WORDS) and not tab[1].any()
    assert tab[0].tolist()[:5] == [0, 0, 39999, 5921, 0] and tab[2].tolist()[:10] == [1, 39999, 0, 0, 0, 60, 4, 116, 28, 60]
    for bad in (dict(push_count=5921, push_src=2 * 5921 + 1), dict(push_count=40001), dict(push_count=1, audio_write=40000),
                dict(ready=1, audio_read=40000), dict(ready=1, audio_read=-1), dict(ready=1, code_write=120), dict(ready=1, seg_valid=117),
                dict(ready=1, emit_row=57, emit_count=60), dict(ready=1, emit_count=61), dict(ready=1, frames=3)):
        with pytest.raises(ValueError):
            ops.stream_table([bad], **GEOMETRY)
    with pytest.raises(ValueError):
        ops.stream_table([dict(push_count=10, push_src=0), dict(push_count=10, push_src=9)], **GEOMETRY)      # two pushes overlap in the staged buffer


@pytest.mark.parametrize("fmt", ["s16", "f32"])
def test_stand_in_rings_equal_numpy_slicing(fmt):
    """Chunks of 5 921 samples into a ring of 40 000: every chunk lands at another offset, odd and even, and the seventh wraps."""
    rng = np.random.default_rng(5)
    pcm = rng.integers(-32768, 32768, 12 * 5921).astype(np.int16)
    want = pcm.astype(np.float32) / np.float32(32768.0)
    src = torch.from_numpy(pcm if fmt == "s16" else want)
    ring, status = torch.full((2, 40000), -7.0), torch.zeros(1, dtype=torch.int32)
    out = torch.full((2, 64 * 533), -7.0)
    for i in range(12):
        tab = ops.stream_table([None, dict(push_count=5921, push_src=0, audio_write=(i * 5921) % 40000)], **GEOMETRY)
        fake_stream_ops.stream_push(src[i * 5921:(i + 1) * 5921].contiguous(), torch.from_numpy(tab), ring, status)
        have = (i + 1) * 5921
        if have >= 64 * 533:
            start = have - 64 * 533                                     # the last 64 frames pushed: a window at any offset
            tab = ops.stream_table([None, dict(ready=1, audio_read=start % 40000)], **GEOMETRY)
            fake_stream_ops.stream_windows(ring, torch.from_numpy(tab), out, status)
            assert np.array_equal(out[1].numpy(), want[start:have]) and not out[0].any(), i
    assert int(status) == 0 and bool((ring[0] == -7.0).all())
    raw = np.zeros((2, ops.STREAM_WORDS), dtype=np.int32)               # rows outside their buffers, the host check bypassed: reported, skipped
    raw[0, [3, 4]] = 5921, 1
    raw[1, [0, 1]] = 1, 40000
    fake_stream_ops.stream_push(src[:5921].contiguous(), torch.from_numpy(raw), ring, status)
    fake_stream_ops.stream_windows(ring, torch.from_numpy(raw), out, status)
    assert int(status) == 3 and bool((ring[0] == -7.0).all()) and not out.any()
