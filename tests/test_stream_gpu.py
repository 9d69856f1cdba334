"""The streaming batch on the MI355X (pantomatrix_amd/streaming.py, csrc/stream.hip):
* the four kernels bit for bit against numpy slicing / the header's restatement (tests/fake_stream_ops.py): rings that wrap at odd and even
  offsets, rows of slots that are not ready, state behind sentinels, rows outside their buffers, and the carried translation against ONE
  `ops.velocity_to_position` over the whole sequence;
* five sessions that start and stop at different times in three slots against the REFERENCE's B = 1 goldens (tests/golden/infer_{F}f_b1.npz):
  code indices identical, poses / expressions / trans within the project's 1e-3, fp32 and f16x3;
* the captured tick against the eager one, bit for bit; a `step()` with nothing ready launches nothing;
* a session's output does not depend on its neighbours, on how its audio is chunked, or on who used its slot before;
* a seeded session against the CPU oracle's `inference(masked_motion=seed)` + decode."""
import numpy as np
import pytest
import torch

import common
import fake_stream_ops as fk
import stream_common as sc
from pantomatrix_amd import ops, streaming, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"
GEOMETRY = dict(ring_len=40000, staged_samples=5921, samples=64 * 533, ring_codes=120, seg_len=116, out_rows=60)


def dev_table(rows, **kw):
    return torch.from_numpy(ops.stream_table(rows, **{**GEOMETRY, **kw})).to(DEV)


# ---- the four kernels ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["s16", "f32"])
def test_push_and_windows_equal_numpy_slicing(fmt):
    """Chunks of 5 921 samples into a ring of 40 000: every chunk lands at another offset, odd and even, and the seventh wraps; the
    windows read back the last 64 frames pushed, so they start at odd and even offsets and wrap too."""
    rng = np.random.default_rng(5)
    pcm = rng.integers(-32768, 32768, 12 * 5921).astype(np.int16)
    want = pcm.astype(np.float32) / np.float32(32768.0)
    src = torch.from_numpy(pcm if fmt == "s16" else want).to(DEV)
    ring, status = torch.full((3, 40000), -7.0, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    out = torch.full((3, 64 * 533 + 3), -7.0, device=DEV)                           # a wider buffer: the columns behind a row keep their contents
    starts = []
    for i in range(12):
        ops.stream_push(src[i * 5921:(i + 1) * 5921], dev_table([None, dict(push_count=5921, push_src=0, audio_write=(i * 5921) % 40000), None]), ring, status)
        have = (i + 1) * 5921
        if have >= 64 * 533:
            start = have - 64 * 533
            starts.append(start % 40000)
            ops.stream_windows(ring, dev_table([None, dict(ready=1, audio_read=start % 40000), None]), out[:, :64 * 533], status)
            got = out.cpu().numpy()
            assert np.array_equal(got[1, :64 * 533], want[start:have]), i
            assert not got[0, :64 * 533].any() and not got[2, :64 * 533].any(), "rows of slots that are not ready are zero"
            assert (got[:, 64 * 533:] == -7.0).all()
    assert {s % 2 for s in starts} == {0, 1} and any(s + 64 * 533 > 40000 for s in starts)
    assert int(status) == 0 and bool((ring[0] == -7.0).all()) and bool((ring[2] == -7.0).all())
    raw = np.zeros((3, ops.STREAM_WORDS), dtype=np.int32)                           # rows outside their buffers, the host check bypassed
    raw[0, [3, 4]] = 5921, 1                                                        # one sample beyond the staged buffer
    raw[1, [0, 1]] = 1, 40000                                                       # a window that starts behind the ring
    raw[2, [2, 3]] = 40000, 8                                                       # a push that lands behind the ring
    before = ring.clone()
    ops.stream_push(src[:5921], torch.from_numpy(raw).to(DEV), ring, status)
    assert int(status) == fk.BAD_PUSH and torch.equal(ring, before)
    ops.stream_windows(ring, torch.from_numpy(raw).to(DEV), out[:, :64 * 533], status)
    assert int(status) == fk.BAD_PUSH | fk.BAD_WINDOW and not out[:, :64 * 533].any()


def test_commit_keeps_the_state_of_slots_that_are_not_ready():
    g = torch.Generator().manual_seed(9)
    win = torch.randint(0, 256, (4, 3, 64), generator=g)
    ring0 = torch.randint(1000, 2000, (4, 3, 120), generator=g)                     # sentinels: no code is that large
    seeds0, dec = torch.randn(3, 4, 337, generator=g), torch.randn(3, 11, 337, generator=g)
    rows = [dict(ready=1, audio_read=0, code_write=0, seg_read=64, seg_valid=116, emit_row=28, emit_count=60),      # window 2: the segment wraps
            dict(push_count=8),                                                                                    # open, audio only: not ready
            dict(ready=1, code_write=0, seg_read=0, seg_valid=60, emit_count=32)]                                  # window 0: left-aligned, 56 rows filled
    tab = ops.stream_table(rows, **GEOMETRY)
    want_ring, want_seeds, want_seg = ring0.clone(), seeds0.clone(), torch.full((4, 3, 116), -1)
    fk.stream_commit(torch.from_numpy(tab), win, 60, want_ring, want_seg, dec[:, 7:], want_seeds, torch.zeros(1, dtype=torch.int32))
    ring, seeds, seg = ring0.to(DEV), seeds0.to(DEV), torch.full((4, 3, 116), -1, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.stream_commit(torch.from_numpy(tab).to(DEV), win.to(DEV), 60, ring, seg, dec.to(DEV)[:, 7:], seeds, status)
    assert int(status) == 0
    assert torch.equal(ring.cpu(), want_ring) and torch.equal(seeds.cpu(), want_seeds) and torch.equal(seg.cpu(), want_seg)
    assert torch.equal(ring[:, 1].cpu(), ring0[:, 1]) and torch.equal(seeds[1].cpu(), seeds0[1]) and not seg[:, 1].any()
    assert torch.equal(seeds[0].cpu(), dec[0, 7:]) and torch.equal(ring[:, 0, :60].cpu(), win[:, 0, :60]) and torch.equal(ring[:, 0, 60:].cpu(), ring0[:, 0, 60:])
    assert torch.equal(seg[:, 2, :60].cpu(), win[:, 2, :60]) and not seg[:, 2, 60:].any()
    raw = tab.copy()                                                                # a code position behind the ring, the host check bypassed
    raw[0, fk.CODE_WRITE] = 120
    before = (ring.clone(), seeds.clone())
    ops.stream_commit(torch.from_numpy(raw).to(DEV), win.to(DEV) + 1, 60, ring, seg, dec.to(DEV)[:, :4], seeds, status)
    assert int(status) == fk.BAD_COMMIT and torch.equal(ring[:, :2], before[0][:, :2]) and torch.equal(seeds[:2], before[1][:2]) and not seg[:, 0].any()


def test_emit_over_consecutive_segments_equals_one_scan():
    """Two slots, 240 frames: the emit ranges of a stream's ticks (32 frames, then 60 at a time), each cut out of a 116-row segment, against
    ONE `ops.velocity_to_position` over the whole sequence — and the rows' poses, expressions and codes against slicing."""
    g = torch.Generator().manual_seed(13)
    s, t = 2, 240
    aa, expr, vel = torch.randn(s, t, 165, generator=g), torch.randn(s, t, 100, generator=g), torch.randn(s, t, 61, generator=g)
    codes = torch.randint(0, 256, (4, s, t), generator=g)
    init = torch.tensor([[0.25, 9.0, -0.5], [-1.0, 9.0, 0.75]])
    whole = ops.velocity_to_position(vel.to(DEV).view(s * t, 61), 54, init.to(DEV), 1 / 30, s, t)
    carry, status = init.to(DEV).clone(), torch.zeros(1, dtype=torch.int32, device=DEV)
    outs = [torch.full((s, 60, w), -7.0, device=DEV) for w in (165, 100, 3)] + [torch.full((s, 60, 4), -7, dtype=torch.int64, device=DEV)]
    got, emitted = [[], [], [], []], 0
    for k in range(3):
        have = 60 * k + 60
        start = max(0, have - 116)
        upto = have - 28
        seg = lambda x: x[:, start:start + 116].contiguous().to(DEV)
        # slot 1 stops after the second tick: not ready, it emits nothing and its carry stays
        rows = [dict(ready=1, emit_row=emitted - start, emit_count=upto - emitted), dict(ready=1, emit_row=emitted - start, emit_count=upto - emitted) if k < 2 else None]
        ops.stream_emit(dev_table(rows), seg(aa).view(-1, 165), seg(expr).view(-1, 100), seg(vel).view(-1, 61), 54, 1 / 30,
                        codes[:, :, start:start + 116].contiguous().to(DEV), carry, *outs, status)
        n = upto - emitted
        for o in outs:
            assert not o[:, n:].any() and (k < 2 or not o[1].any()), "rows beyond the count are zero"
        for acc, o in zip(got, outs):
            acc.append(o[:, :n].cpu().clone())
        emitted = upto
    assert int(status) == 0 and emitted == 152
    poses, expressions, trans, cds = (torch.cat(x, dim=1) for x in got)
    assert torch.equal(trans[0], whole[0, :152].cpu()) and torch.equal(trans[1, :92], whole[1, :92].cpu())
    assert torch.equal(poses[0], aa[0, :152]) and torch.equal(expressions[0], expr[0, :152]) and torch.equal(cds[0], codes[:, 0, :152].T)
    assert torch.equal(carry[0, [0, 2]].cpu(), whole[0, 152, [0, 2]].cpu()) and torch.equal(carry[1, [0, 2]].cpu(), whole[1, 92, [0, 2]].cpu())
    assert float(carry[0, 1]) == 9.0                                                # the height is decoded, not carried
    raw = ops.stream_table([dict(ready=1, emit_row=0, emit_count=60), None], **GEOMETRY)
    raw[0, fk.EMIT_ROW] = 57                                                        # rows 57 .. 116 of a 116-row segment
    before = carry.clone()
    ops.stream_emit(torch.from_numpy(raw).to(DEV), seg(aa).view(-1, 165), seg(expr).view(-1, 100), seg(vel).view(-1, 61), 54, 1 / 30,
                    codes[:, :, :116].contiguous().to(DEV), carry, *outs, status)
    assert int(status) == fk.BAD_EMIT and torch.equal(carry, before) and not any(bool(o.any()) for o in outs)


# ---- sessions ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models():
    return {p: common.product_models(precision=p, device=DEV) for p in ("fp32", "f16x3")}


def make_batch(models, precision, use_graph=False):
    """Three slots; max_seconds = 11 with max_push = 48 000 gives a ring of 82 234 samples, which the longest waveform wraps twice."""
    sb = streaming.StreamBatch(*models[precision], slots=3, max_seconds=11, use_graph=use_graph)
    assert sb.ring_len == 82234 and sb.lag == 28
    return sb


@pytest.fixture(scope="module")
def eager(models):
    """The scenario through an EAGER batch per precision -> {precision: (batch, results)}; computed once, read-only."""
    out = {}
    for p in models:
        sb = make_batch(models, p)
        out[p] = (sb, sc.scenario(sb, sc.waves()))
    return out


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", list("ABCDE"))
def test_sessions_match_the_reference_goldens(eager, golden_dir, precision, name):
    sc.check_against_golden(name, eager[precision][1][name], golden_dir, precision)


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and all(np.array_equal(a[3][p], b[3][p]) for p in a[3])


class _Count:
    def __init__(self):
        self.n = 0

    def tag(self):
        return ""

    def fire(self, kind, entries, launch):
        self.n += 1
        return launch()

    def replay(self):
        self.n += 1


def test_captured_batch_equals_the_eager_one(models, eager):
    sb = make_batch(models, "f16x3", use_graph=True)
    assert sb.graph is not None
    got = sc.scenario(sb, sc.waves())
    for name in "ABCDE":
        assert same(got[name], eager["f16x3"][1][name]), name
    # nothing ready: no replay, no launch, nothing copied — in the captured batch and in the eager one
    s = sb.open()
    s.push(sc.waves(names="E")["E"][:20000])
    graph, counter = sb.graph, _Count()
    sb.graph, ops._TRACE[0] = counter, counter
    try:
        assert sb.step() == {} and eager["f16x3"][0].step() == {} and counter.n == 0
    finally:
        sb.graph, ops._TRACE[0] = graph, None
    assert len(s._staged) == 1                                                     # what was pushed waits on the host
    s.close()


def test_a_session_does_not_depend_on_neighbours_chunking_or_slot_history(models, eager):
    w = sc.waves(names="A")["A"]
    want = sc.run_alone(make_batch(models, "f16x3"), w)                            # slot 0 of a FRESH batch, the other slots idle
    assert same(want, eager["f16x3"][1]["A"])                                      # the scenario's A had C, E, B and D beside it
    sb = eager["f16x3"][0]                                                         # a batch whose slots other sessions have used
    assert same(sc.run_alone(sb, w, chunk=1000), want)
    other = sc.waves(seed=99, names="BC")
    a, b, c = sb.open(), sb.open(), sb.open()                                      # other audio in slots 1 and 2, one window ahead of A's
    assert a.slot == 0
    for s, k in ((b, "B"), (c, "C")):
        sc.feed_window(s, other[k])
    assert set(sb.step()) == {b, c}
    sc.feed_window(b, other["B"])
    assert same(sc.run_alone(sb, w, session=a), want) and b.windows == 2
    b.close(), c.close()


def test_non_finite_audio_raises(models):
    sb = make_batch(models, "f16x3")
    s = sb.open()
    s.push(np.full(streaming.window_need(0), np.nan, dtype=np.float32))
    with pytest.raises(FloatingPointError):
        sb.step()


def test_s16_batch_equals_the_f32_batch_on_the_same_samples(models, eager):
    """70 frames (one window and a tail) as int16 PCM through an 's16' batch, and as the same values x * 2^-15 through the f32 one."""
    pcm = np.round(sc.waves(names="C")["C"] * 32768.0).clip(-32768, 32767).astype(np.int16)
    sb = streaming.StreamBatch(*models["f16x3"], slots=3, audio_format="s16", max_seconds=11, use_graph=False)
    with pytest.raises(ValueError):
        sb.open().push(pcm.astype(np.float32))
    sb.sessions[0].close()
    got = sc.run_alone(sb, pcm, chunk=5921)
    want = sc.run_alone(eager["f16x3"][0], pcm.astype(np.float32) / np.float32(32768.0))
    assert got[0].shape == (70, 165) and same(got, want)
    assert same(sc.run_alone(eager["f16x3"][0], pcm), want)                        # int16 chunks into an f32 batch: decoded on the host


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_seeded_session_matches_the_oracle(models, precision):
    from oracle import emage_oracle as orc
    omodel, ovq = common.oracle_models()
    wave = synthetic.synthetic_audio(1, synthetic.samples_for_frames(129), seed=6)[0]
    g = torch.Generator().manual_seed(17)
    aa = 0.2 * torch.randn(4, 55, 3, generator=g)
    seed = torch.cat([orc.axis_angle_to_rotation_6d(aa).reshape(4, 330), 0.05 * torch.randn(4, 7, generator=g)], dim=-1)
    ref_trans = torch.tensor([-1.0, 0.5, 0.75])
    sb = make_batch(models, precision)
    poses, expressions, trans, codes = sc.run_alone(sb, wave.numpy(), seed=seed, ref_trans=ref_trans)
    with torch.no_grad():
        ref = omodel.inference(wave[None], torch.zeros(1, 1, dtype=torch.long), ovq, masked_motion=seed[None])
        sel = omodel.select_codes(ref)
        rdec = ovq.decode(**sel, get_global_motion=True, ref_trans=ref_trans[None])
    for p in ("upper", "hands", "lower"):
        assert np.array_equal(codes[p], sel[f"{p}_index"][0].numpy()), p
    for nm, got, key in (("poses", poses, "motion_axis_angle"), ("expressions", expressions, "expression"), ("trans", trans, "trans")):
        err = float(np.abs(got - rdec[key][0].numpy()).max())
        print(f"{precision} seeded 129f {nm}: max|err| {err:.2e}")
        assert got.shape[0] == 129 and err < sc.TOL, (nm, err)
    assert float(trans[0, 0]) == -1.0 and float(trans[0, 2]) == 0.75
