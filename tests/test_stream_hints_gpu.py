"""Motion hints in live stream sessions on the MI355X (csrc/stream.hip: emage_stream_push_hints; pantomatrix_amd/streaming.py rule 5):
* the kernel bit for bit against the header's restatement (tests/fake_stream_hint_ops.py: `ring_model`) in the smallest ring (3 slots, 120
  rows, C = 337, ld = 344): pushes that land mid-ring, wrap and cover the mirrored rows, slots without a push behind sentinels, the tracker
  form against `ops.axis_angle_to_rot6d`, the seed rows, the window table, rows outside their buffers, and `ops.pack_motion_hints` over ring
  and window table against `ops.pack_motion` over the dense windows in every storage dtype;
* the five-session scenario, every session hinted, against the REFERENCE's hinted B = 1 goldens (tests/golden/infer_hints_{F}f_b1.npz):
  code indices identical, poses / expressions / trans within the project's 1e-3, fp32 and f16x3;
* the captured batch against the eager one, and a second scenario with other hints on the same graph against `RecordingRunner(hints=True)`;
* a hinted session does not depend on its hints' chunking, its slot's history or hinted neighbours; a plain session in a hinted batch equals
  the plain batch; the tracker form equals the packed form; rule 5's gating."""
import numpy as np
import pytest
import torch

import common
import fake_stream_hint_ops as fh
import stream_common as sc
import stream_hints_common as shc
import test_recording_hints_gpu as trh
from pantomatrix_amd import ops, recordings as R, streaming

pytestmark = pytest.mark.gpu
DEV = "cuda"
SLOTS, HINT_ROWS, C, LD = 3, 120, 337, 344


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------------
class Rings:
    """The device state of a 3-slot batch behind sentinels, and the numpy model of it."""

    def __init__(self):
        g = np.random.default_rng(1)
        self.host = dict(ring_m=np.full((SLOTS, HINT_ROWS + 4, LD), -7.0, np.float32), ring_k=np.full((SLOTS, HINT_ROWS + 4, LD), 9, np.uint8),
                         seeds=g.standard_normal((SLOTS, 4, C)).astype(np.float32), wt=np.full((SLOTS, 2), -1, np.int64))
        self.dev = {k: torch.from_numpy(v.copy()).to(DEV) for k, v in self.host.items()}
        self.status = torch.zeros(1, dtype=torch.int32, device=DEV)

    def launch(self, staged, table, rot6d=None):
        """One launch on the device and in the model -> the model's status bits; asserts the device state equals the model's bit for bit."""
        d, h = self.dev, self.host
        ops.stream_push_hints(torch.from_numpy(staged).to(DEV), torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32)).to(DEV), d["ring_m"],
                              d["ring_k"], d["seeds"], d["wt"], 64, self.status)
        bits = fh.ring_model(staged, table, h["ring_m"], h["ring_k"], h["seeds"], h["wt"], 64, rot6d)
        for k in h:
            got = d[k].cpu().numpy()
            assert np.array_equal(got.view(np.uint8), h[k].view(np.uint8)), k
        return bits

    def push(self, rows, chunks, rot6d=None):
        """rows: per slot None or a dict without `src`; chunks: per slot None or (form, motion, mask)."""
        staged, offsets = fh.stage([c for c in chunks if c is not None])
        it = iter(offsets)
        rows = [None if r is None else ({**r, "src": next(it)} if r.get("frames") else r) for r in rows]
        return self.launch(staged, ops.stream_hint_table(rows, hint_rows=HINT_ROWS, staged_bytes=staged.size), rot6d)


def frames_of(n, seed=0):
    g = np.random.default_rng(seed)
    return g.standard_normal((n, C)).astype(np.float32), g.integers(0, 2, (n, C)).astype(np.uint8)


def test_pushes_land_wrap_and_mirror_and_idle_slots_keep_their_bits():
    """Slot 1: 1, 7 and 64 frames from frame 50 on (mid-ring; the third wraps at row 119 -> 0 and covers rows 0, 1 and their mirrors), then 7
    frames that cover rows 2 .. 8; slots 0 and 2 have no push: every byte of theirs stays a sentinel."""
    r = Rings()
    motion, keep = frames_of(200)
    at = 50
    for n in (1, 7, 64, 7):
        assert r.push([None, dict(frames=n, form=0, frames_before=at), None], [None, (0, motion[at:at + n], keep[at:at + n]), None]) == 0
        at += n
    ring_m, ring_k = r.dev["ring_m"].cpu().numpy(), r.dev["ring_k"].cpu().numpy()
    for f in range(50, 129):
        assert np.array_equal(ring_m[1, f % 120, :C], motion[f]) and np.array_equal(ring_k[1, f % 120, :C], keep[f]), f
    for f in range(120, 124):                                                       # the mirror of rows 0 .. 3
        assert np.array_equal(ring_m[1, f, :C], motion[f]) and np.array_equal(ring_k[1, f, :C], keep[f]) and not ring_m[1, f, C:].any()
    assert (ring_m[1, 9:50] == -7.0).all() and (ring_m[[0, 2]] == -7.0).all() and (ring_k[[0, 2]] == 9).all()
    assert torch.equal(r.dev["seeds"].cpu(), torch.from_numpy(r.host["seeds"])) and int(r.status) == 0
    assert np.array_equal(r.host["seeds"], Rings().host["seeds"])                   # frames >= 4 never reach the seed rows, rows 0 .. 3 of the ring or not
    assert not r.dev["wt"].any()


def test_seed_rows_take_frames_below_four_only():
    r = Rings()
    before = r.host["seeds"].copy()
    motion, keep = frames_of(12, seed=2)
    assert r.push([dict(frames=7, form=0, frames_before=0), dict(frames=1, form=0, frames_before=2), dict(frames=5, form=0, frames_before=4)],
                  [(0, motion[:7], keep[:7]), (0, motion[2:3], keep[2:3]), (0, motion[4:9], keep[4:9])]) == 0
    seeds = r.dev["seeds"].cpu().numpy()
    assert np.array_equal(seeds[0], motion[:4])
    assert np.array_equal(seeds[1, 2], motion[2]) and np.array_equal(seeds[1, [0, 1, 3]], before[1, [0, 1, 3]])
    assert np.array_equal(seeds[2], before[2]) and int(r.status) == 0


def test_tracker_form_holds_the_bits_of_axis_angle_to_rot6d():
    r = Rings()
    g = np.random.default_rng(4)
    n = 9
    data = np.concatenate([0.4 * g.standard_normal((n, 165)), g.standard_normal((n, 7))], axis=1).astype(np.float32)
    data[1, :165] = 0.0                                                             # the zero rotation: the small-angle branch
    data[2, :3] = 1e-7
    keep = g.integers(0, 2, (n, C)).astype(np.uint8)
    want = ops.axis_angle_to_rot6d(torch.from_numpy(data[:, :165].reshape(n, 55, 3).copy()).to(DEV)).cpu().numpy().reshape(n, 330)
    rot6d = lambda aa: ops.axis_angle_to_rot6d(torch.from_numpy(aa).to(DEV)).cpu().numpy()
    assert r.push([None, None, dict(frames=n, form=1, frames_before=116)], [None, None, (1, data, keep)], rot6d) == 0      # wraps: rows 116 .. 119, 0 .. 4
    ring_m = r.dev["ring_m"].cpu().numpy()
    rows = [(116 + j) % 120 for j in range(n)]
    assert np.array_equal(ring_m[2, rows, :330].view(np.int32), want.view(np.int32)) and np.array_equal(ring_m[2, rows, 330:C], data[:, 165:])
    assert np.array_equal(ring_m[2, 120:124, :330].view(np.int32), want[4:8].view(np.int32))
    assert np.array_equal(want[1], np.tile(np.array([1, 0, 0, 0, 1, 0], np.float32), 55))
    # frames 0 .. 3 of a session in the tracker form: the seed rows hold the converted bits too
    assert r.push([dict(frames=n, form=1, frames_before=0), None, None], [(1, data, keep), None, None], rot6d) == 0
    assert np.array_equal(r.dev["seeds"][0].cpu().numpy()[:, :330].view(np.int32), want[:4].view(np.int32))


def test_window_table_names_ready_hinted_slots_only():
    r = Rings()
    motion, keep = frames_of(64, seed=5)
    # slot 0: ready, window 1 of 130 frames held (rows 60 .. 123, all there); slot 1: a push, not ready; slot 2: no row (an unhinted slot)
    assert r.push([dict(frames_before=130, ready=1, window_index=1), dict(frames=3, form=0, frames_before=7), None], [None, (0, motion[:3], keep[:3]), None]) == 0
    assert r.dev["wt"].cpu().tolist() == [[60, 64], [0, 0], [0, 0]]
    # avail cut by the end of the hints: window 1 with 100 frames held reads 40; window 2 (row 0) with 57 + 64 held reads 1; window 3 reads none
    assert r.push([dict(frames_before=100, ready=1, window_index=1), dict(frames=64, form=0, frames_before=57, ready=1, window_index=2),
                   dict(frames_before=150, ready=1, window_index=3)], [None, (0, motion, keep), None]) == 0
    assert r.dev["wt"].cpu().tolist() == [[60, 40], [124, 1], [2 * 124 + 60, 0]] and int(r.status) == 0


def test_rows_outside_their_buffers_write_nothing():
    """Table rows the host would never build (`ops.stream_hint_table` bypassed): each is skipped and reported; a good row beside them is served."""
    r = Rings()
    motion, keep = frames_of(8, seed=6)
    staged, _ = fh.stage([(0, motion, keep)])
    good = ops.stream_hint_table([dict(frames=8, src=0, form=0, frames_before=0, ready=1, window_index=0)], hint_rows=HINT_ROWS, staged_bytes=staged.size)[0]
    word = dict(count=fh.COUNT, src16=fh.SRC16, form=fh.FORM, write=fh.WRITE, seed_row=fh.SEED_ROW, seed_count=fh.SEED_COUNT, first=fh.WIN_FIRST, avail=fh.WIN_AVAIL)
    bad = [dict(count=9), dict(src16=1), dict(src16=-1), dict(count=121), dict(count=-1), dict(form=2), dict(write=120, seed_count=0), dict(write=-1, seed_count=0),
           dict(seed_row=1), dict(seed_count=5), dict(seed_count=-1), dict(first=61), dict(first=-1), dict(avail=65), dict(avail=-1)]
    while len(bad) % 2:
        bad.append(bad[0])
    for a, b in zip(bad[0::2], bad[1::2]):
        before = {k: v.clone() for k, v in r.dev.items()}
        table = np.stack([good.copy(), good.copy(), good.copy()])
        for row, change in ((table[0], a), (table[2], b)):
            for k, v in change.items():
                row[word[k]] = v
        r.status.zero_()
        assert r.launch(staged, table) == fh.BAD_HINTS and int(r.status) == fh.BAD_HINTS, (a, b)
        for k in ("ring_m", "ring_k", "seeds"):
            assert torch.equal(r.dev[k][[0, 2]], before[k][[0, 2]]), (k, a, b)
        assert r.dev["wt"].cpu().tolist() == [[0, 0], [124, 8], [0, 0]]
        assert np.array_equal(r.dev["ring_m"][1, :8, :C].cpu().numpy(), motion)


@pytest.mark.parametrize("seeded", [False, True])
@pytest.mark.parametrize("name", list(trh.DTYPES))
def test_packing_through_the_ring_equals_pack_motion_on_the_dense_windows(name, seeded):
    """Slot 0 runs window 1 (rows 60 .. 123: its last four are the mirror rows), slot 1 window 2 (row 0 again) cut to 17 frames by the end of
    its hints, slot 2 is unhinted: `pack_motion_hints` over rings + window table against `pack_motion` over the dense (3, 64, 337) windows."""
    dtype = trh.DTYPES[name]()
    r = Rings()
    m0, k0 = frames_of(124, seed=7)
    m1, k1 = frames_of(137, seed=8)
    assert r.push([dict(frames=64, form=0, frames_before=0), dict(frames=77, form=0, frames_before=0), None], [(0, m0[:64], k0[:64]), (0, m1[:77], k1[:77]), None]) == 0
    assert r.push([dict(frames=60, form=0, frames_before=64, ready=1, window_index=1), dict(frames=60, form=0, frames_before=77, ready=1, window_index=2), None],
                  [(0, m0[64:], k0[64:]), (0, m1[77:], k1[77:]), None]) == 0
    assert r.dev["wt"].cpu().tolist() == [[60, 64], [124, 17], [0, 0]]
    g = torch.Generator().manual_seed(11)
    emb = torch.randn(C, generator=g).to(DEV)
    seed = torch.randn(3, 4, C, generator=g).to(DEV) if seeded else None
    dense_m, dense_k = torch.zeros(3, 64, C), torch.ones(3, 64, C)
    dense_m[0], dense_k[0] = torch.from_numpy(m0[60:124]), torch.from_numpy(k0[60:124]).float()
    dense_m[1, :17], dense_k[1, :17] = torch.from_numpy(m1[120:137]), torch.from_numpy(k1[120:137]).float()
    got = ops.pack_motion_hints(dtype, r.dev["ring_m"].view(-1, LD)[:, :C], r.dev["ring_k"].view(-1, LD)[:, :C], r.dev["wt"], emb, 344, 64, r.status, seed=seed)
    want = ops.pack_motion(dtype, dense_m.to(DEV), dense_k.to(DEV), emb, 344, seed=seed)
    assert int(r.status) == 0 and got.shape == (3 * 64, 344) and torch.equal(trh.bits(got), trh.bits(want))
    # the unhinted slot's rows are what the templates of a batch without hints pack
    tmpl = ops.pack_motion(dtype, R.identity_seed(1, 64).to(DEV), torch.ones(1, 64, C, device=DEV), emb, 344, seed=None if seed is None else seed[2:])
    assert torch.equal(trh.bits(got[128:]), trh.bits(tmpl))


# ---- sessions ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models():
    return {p: common.product_models(precision=p, device=DEV) for p in ("fp32", "f16x3")}


def make_batch(models, precision, use_graph=False, motion_hints=True):
    """Three slots; max_hint_push = 90 gives a ring of 180 rows: in the 310-frame golden, frame 183 (every column given, a seed frame of
    window 3) sits in a mirror row for window 2 and in row 3 for window 3."""
    sb = streaming.StreamBatch(*models[precision], slots=3, max_seconds=11, use_graph=use_graph, motion_hints=motion_hints, max_hint_push=90)
    assert sb.ring_len == 82234 and sb.lag == 28 and (not motion_hints or sb.hint_rows == 180)
    return sb


@pytest.fixture(scope="module")
def hints(golden_dir):
    h = shc.golden_hints(golden_dir)
    assert {k: shc.hint_length(v) for k, v in h.items()} == shc.HINT_FRAMES and not h["A"][1][183].any() and h["A"][1][184].all()
    return h


@pytest.fixture(scope="module")
def eager(models, hints):
    """The hinted scenario through an EAGER batch per precision -> {precision: (batch, results)}; computed once, read-only."""
    out = {}
    for p in models:
        sb = make_batch(models, p)
        out[p] = (sb, shc.scenario(sb, sc.waves(), hints)[0])
    return out


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", list("ABCDE"))
def test_hinted_sessions_match_the_reference_goldens(eager, golden_dir, precision, name):
    got = eager[precision][1][name]
    shc.check_against_golden(name, got, golden_dir, precision)
    if name == "B":                                                                # motion=True, no hints, ended at once: what it generates alone
        plain = np.load(f"{golden_dir}/infer_129f_b1.npz")
        for p in sc.PARTS:
            assert np.array_equal(got[3][p], plain[f"index_{p}"][0]), p


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and all(np.array_equal(a[3][p], b[3][p]) for p in a[3])


def test_captured_batch_equals_the_eager_one_and_replays_other_hints(models, eager, hints):
    model, vq = models["f16x3"]
    sb = make_batch(models, "f16x3", use_graph=True)
    graph = sb.graph
    assert graph is not None
    got, sessions = shc.scenario(sb, sc.waves(), hints)
    for name in "ABCDE":
        assert same(got[name], eager["f16x3"][1][name]), name
    assert all(s.hint_frames_unused == 0 for s in sessions.values())
    # other hints of other prefix lengths and other parts, same graph: every session against the eager offline hinted pass, code for code
    motions, masks = trh.other_hints()                                              # in the order of the recordings test: 70, 310, 40, 129, 64 frames
    names = "CAEBD"
    other = {n: (motions[i], masks[i]) for i, n in enumerate(names)}
    w = sc.waves()
    got, _sessions = shc.scenario(sb, w, other, hint_chunk=25)
    assert sb.graph is graph
    rs = R.RecordingSet.from_audio([torch.from_numpy(w[n]) for n in names], DEV, masked_motion=motions, mask=masks)
    runner = R.RecordingRunner.for_set(model, vq, rs, use_graph=False)
    results = runner(rs)
    for i, n in enumerate(names):
        for p, v in runner.codes_of(i).items():
            assert np.array_equal(got[n][3][p], v.cpu().numpy()), (n, p)
        for x, y in zip(got[n][:3], results[i]):
            assert float(np.abs(x - y).max()) < sc.TOL, n
    assert not same(got["A"], eager["f16x3"][1]["A"])


def test_a_hinted_session_does_not_depend_on_chunking_slot_history_or_hinted_neighbours(models, eager, hints):
    w = sc.waves(names="A")["A"]
    want = shc.run_alone(make_batch(models, "f16x3"), w, hints["A"])               # slot 0 of a FRESH batch, whole windows of hints
    assert same(want, eager["f16x3"][1]["A"])                                      # the scenario's A had hinted C, E, B and D beside it
    sb = eager["f16x3"][0]                                                         # a batch whose slots held hinted sessions before
    assert same(shc.run_alone(sb, w, hints["A"], chunk=1000, hint_chunk=7), want)
    motions, masks = trh.other_hints()
    other_w = sc.waves(seed=99, names="BC")
    a, b, c = sb.open(motion=True), sb.open(motion=True), sb.open(motion=True)     # other audio, other hints in slots 1 and 2, one window ahead of A's
    assert a.slot == 0
    nb = {"B": (motions[3], masks[3]), "C": (motions[2], masks[2])}                # 129 frames, the upper body late; 40 frames, the lower body
    for s, k in ((b, "B"), (c, "C")):
        sc.feed_window(s, other_w[k]), shc.feed_hints(s, nb[k])
    assert set(sb.step()) == {b, c}
    sc.feed_window(b, other_w["B"]), shc.feed_hints(b, nb["B"])
    assert same(shc.run_alone(sb, w, hints["A"], session=a), want) and b.windows == 2
    b.close(), c.close()


def test_a_plain_session_in_a_hinted_batch_equals_the_plain_batch(models, eager):
    w = sc.waves(names="A")["A"]
    want = sc.run_alone(make_batch(models, "f16x3", motion_hints=False), w)
    assert same(sc.run_alone(eager["f16x3"][0], w), want)                          # slot 0 held the hinted A: its ring still holds A's frames
    assert not same(want, eager["f16x3"][1]["A"])


def test_tracker_form_equals_the_packed_form(models, eager):
    """70 frames, the upper body and the root translation kept from a 'capture': pushed as axis-angle poses (converted on the device) and as
    the rot6d `ops.axis_angle_to_rot6d` gives for the same poses."""
    sb = eager["f16x3"][0]
    w = sc.waves(names="C")["C"]
    g = torch.Generator().manual_seed(31)
    poses = (0.3 * torch.randn(70, 165, generator=g)).numpy()
    rot6d = ops.axis_angle_to_rot6d(torch.from_numpy(poses).view(70, 55, 3).to(DEV)).cpu().numpy().reshape(70, 330)
    motion = np.concatenate([rot6d, 0.05 * torch.randn(70, 3, generator=g).numpy(), torch.randint(0, 2, (70, 4), generator=g).float().numpy()], axis=1)
    mask = np.ones((70, C), np.uint8)
    mask[:, np.concatenate([R.part_columns("upper"), R.part_columns("trans")])] = 0
    packed = shc.run_alone(sb, w, (motion, mask), hint_chunk=30)
    tracker = shc.run_alone(sb, w, (motion, mask), hint_chunk=30, poses=poses)
    assert packed[0].shape == (70, 165) and same(tracker, packed)
    assert not same(packed, eager["f16x3"][1]["C"])


def test_windows_wait_for_their_hint_frames(models, eager, hints):
    sb = eager["f16x3"][0]
    w = sc.waves(names="B")["B"]
    motion, mask = hints["A"]
    with pytest.raises(ValueError, match="not both"):
        sb.open(seed=torch.zeros(4, C), motion=True)
    s = sb.open(motion=True)
    sc.feed_window(s, w)
    s.push_motion(motion[:63], mask[:63])
    assert s.waiting == "motion" and not s.ready and sb.step() == {}                # the audio is there, frame 63 is not
    s.push_motion(motion[63:64], mask[63:64])
    assert s.waiting is None and list(sb.step()) == [s] and s.windows == 1
    sc.feed_window(s, w)
    s.push_motion(motion[64:100], mask[64:100])
    assert s.waiting == "motion" and sb.step() == {}
    with pytest.raises(RuntimeError, match="pending"):
        s.close()                                                                   # close() ends the hints: window 1 is pending
    assert s.hints_ended and list(sb.step()) == [s] and s.windows == 2
    sc.feed(s, w, len(w))
    out = s.close()                                                                 # frames 92 .. 128: the tail window reads no hints (100 < 120)
    assert out.poses.shape[0] == 37 and s.emitted == 129 and s.hint_frames_unused == 0
    s = sb.open(motion=True)
    s.push_motion(motion[:180], mask[:180])                                         # the whole ring
    with pytest.raises(ValueError, match="do not fit"):
        s.push_motion(motion[180:181], mask[180:181])
    s._hint_staged = []                                                             # dropped: nothing of it reached the device
    s.close()
