"""Shared by the stream-hint tests (host and GPU): the hints of tests/golden/infer_hints_{F}f_b1.npz per session name of
`stream_common.FRAMES`, a feeder that pushes a session's hints window by window (rule 5: up to 60 * windows + 64 frames before each tick)
and ends them once the prefix is exhausted, and `stream_common.scenario` rerun with every session hinted."""
import os

import numpy as np

import stream_common as sc

C = 337
HINT_FRAMES = dict(A=200, B=0, C=70, D=20, E=10)         # the goldens' prefix lengths (test_recording_hints_gpu.py: rs.hint_len)


def golden_hints(golden_dir):
    """-> {name: (masked_motion or None, mask or None)}: what the reference's B = 1 call of each golden was given."""
    out = {}
    for name, f in sc.FRAMES.items():
        g = np.load(os.path.join(golden_dir, f"infer_hints_{f}f_b1.npz"))
        out[name] = (g["hint_motion"] if bool(g["has_motion"]) else None, g["hint_keep"] if bool(g["has_mask"]) else None)
    return out


def hint_length(hints):
    return max(0 if a is None else len(a) for a in hints)


def push_range(session, hints, lo, hi, poses=None):
    """Frames [lo, hi) of (motion, mask) prefixes of possibly different lengths: one push per stretch in which the same arrays exist.
    poses: (h, 165) axis-angle behind the motion's rot6d columns — the stretch is then pushed in the tracker form."""
    motion, mask = hints
    cuts = sorted({lo, hi} | {len(a) for a in hints if a is not None and lo < len(a) < hi})
    for a, b in zip(cuts, cuts[1:]):
        m = motion[a:b] if motion is not None and b <= len(motion) else None
        k = mask[a:b] if mask is not None and b <= len(mask) else None
        if m is not None and poses is not None:
            session.push_motion(mask=k, poses=poses[a:b], trans=m[:, 330:333], contact=m[:, 333:])
        else:
            session.push_motion(m, k)


def feed_hints(session, hints, chunk=None, poses=None):
    """Push the session's hints up to the frames its next window needs (60 * windows + 64), in pieces of `chunk` frames (None: one piece),
    and end them once the prefix is exhausted."""
    h = hint_length(hints)
    lo, upto = session.hint_frames, min(h, 60 * session.windows + 64)
    step = max(upto - lo, 1) if chunk is None else chunk
    while lo < upto:
        push_range(session, hints, lo, min(lo + step, upto), poses)
        lo = min(lo + step, upto)
    if session.hint_frames >= h and not session.hints_ended:
        session.end_motion()


def run_alone(sb, wave, hints, chunk=None, hint_chunk=None, session=None, poses=None):
    """`stream_common.run_alone` for a hinted session."""
    s = sb.open(motion=True) if session is None else session
    pieces = []
    while True:
        sc.feed_window(s, wave, chunk), feed_hints(s, hints, hint_chunk, poses)
        out = sb.step()
        if s not in out:
            break
        pieces.append(out[s])
    pieces.append(s.close())
    return sc.joined(pieces)


def scenario(sb, w, hints, chunk=None, hint_chunk=None):
    """`stream_common.scenario` with every session opened with motion=True and fed `hints[name]`: S = 3, slots reused -> {name: joined
    output}, and the sessions (for their counters)."""
    acc = {k: [] for k in "ABCDE"}
    fh = lambda s, name: feed_hints(s, hints[name], hint_chunk)
    a, c, e = sb.open(motion=True), sb.open(motion=True), sb.open(motion=True)
    assert (a.slot, c.slot, e.slot) == (0, 1, 2)
    sc.feed_window(a, w["A"], chunk), sc.feed(c, w["C"], len(w["C"]), chunk), sc.feed(e, w["E"], len(w["E"]), chunk)
    fh(a, "A"), fh(c, "C"), fh(e, "E")
    acc["E"].append(e.close())                                                     # a recording that is only a tail: hints and all in close()
    out = sb.step()
    assert set(out) == {a, c} and a.windows == 1
    acc["A"].append(out[a]), acc["C"].append(out[c])
    b = sb.open(motion=True)
    assert b.slot == 2
    sc.feed_window(b, w["B"], chunk), sc.feed_window(a, w["A"], chunk)
    fh(b, "B"), fh(a, "A"), fh(c, "C")                                              # C's last frames: hints of its tail, pushed just before close()
    acc["C"].append(c.close())
    d = sb.open(motion=True)
    assert d.slot == 1
    sc.feed(d, w["D"], len(w["D"]), chunk), fh(d, "D")
    out = sb.step()                                                                # A in window 1, B and D in window 0
    assert set(out) == {a, b, d}
    acc["A"].append(out[a]), acc["B"].append(out[b]), acc["D"].append(out[d])
    acc["D"].append(d.close())
    while True:
        sc.feed_window(a, w["A"], chunk), sc.feed_window(b, w["B"], chunk)
        fh(a, "A"), fh(b, "B")
        out = sb.step()
        if not out:
            break
        for s, name in ((a, "A"), (b, "B")):
            if s in out:
                acc[name].append(out[s])
    acc["A"].append(a.close()), acc["B"].append(b.close())
    assert (a.windows, b.windows, c.windows, d.windows, e.windows) == (5, 2, 1, 1, 0)
    return {k: sc.joined(v) for k, v in acc.items()}, dict(A=a, B=b, C=c, D=d, E=e)


def check_against_golden(name, got, golden_dir, label=""):
    """Code indices identical to the reference's hinted B = 1 golden of the same waveform and hints, arrays within `stream_common.TOL`."""
    g = np.load(os.path.join(golden_dir, f"infer_hints_{sc.FRAMES[name]}f_b1.npz"))
    assert float(g["gap_logit"]) >= float(g["gap_logit_unhinted"]) and float(g["gap_distance"]) >= float(g["gap_distance_unhinted"])
    poses, expressions, trans, codes = got
    n = sc.FRAMES_OUT[name]
    assert poses.shape == (n, 165) and expressions.shape == (n, 100) and trans.shape == (n, 3) and g["poses"].shape == (1, n, 165)
    for p in sc.PARTS:
        assert np.array_equal(codes[p], g[f"index_{p}"][0]), f"{name}: {p} code indices differ"
    for nm, x in (("poses", poses), ("expressions", expressions), ("trans", trans)):
        err = float(np.abs(x - g[nm][0]).max())
        print(f"{label} hinted {name} ({sc.FRAMES[name]}f) {nm}: max|err| {err:.2e}")
        assert err < sc.TOL, (name, nm, err)
