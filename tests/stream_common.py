"""Shared by the stream tests (host and GPU): the five waveforms of tests/golden/infer_{F}f_b1.npz, a feeder that pushes a session's audio
window by window, and the five-session scenario in which sessions start and stop at different times and slots are reused."""
import os

import numpy as np

from pantomatrix_amd import streaming, synthetic

FRAMES = dict(A=310, B=129, C=70, D=64, E=40)
FRAMES_OUT = dict(A=310, B=129, C=70, D=60, E=40)
PARTS = ("face", "upper", "hands", "lower")
TOL = 1e-3                                               # the project's parity tolerance (test_parity_gpu.py)


def waves(seed=1234, names="ABCDE"):
    return {k: synthetic.synthetic_audio(1, synthetic.samples_for_frames(FRAMES[k]), seed=seed)[0].numpy() for k in names}


def feed(session, wave, upto, chunk=None):
    """Push wave[session.pushed : upto] in pieces of `chunk` samples (None: one piece)."""
    lo, upto = session.pushed, min(int(upto), len(wave))
    step = upto - lo if chunk is None else chunk
    while lo < upto:
        session.push(wave[lo:min(lo + step, upto)])
        lo = min(lo + step, upto)


def feed_window(session, wave, chunk=None):
    """Push what the session's next window needs — or, when the waveform ends before that, the rest of it."""
    feed(session, wave, streaming.window_need(session.windows), chunk)


def joined(pieces):
    """[Emitted] -> (poses, expressions, trans, {part: codes}) concatenated."""
    cat = lambda xs: np.concatenate(xs, axis=0)
    return (cat([e.poses for e in pieces]), cat([e.expressions for e in pieces]), cat([e.trans for e in pieces]),
            {p: cat([e.codes[p] for e in pieces]) for p in pieces[0].codes})


def run_alone(sb, wave, chunk=None, session=None, **open_kw):
    """One session (a new one, or `session`) fed window by window until it closes -> joined output.  Other open sessions tick along."""
    s = sb.open(**open_kw) if session is None else session
    pieces = []
    while True:
        feed_window(s, wave, chunk)
        out = sb.step()
        if s not in out:
            break
        pieces.append(out[s])
    pieces.append(s.close())
    return joined(pieces)


def scenario(sb, w, chunk=None):
    """S = 3.  A (310), C (70) and E (40) open; E closes at once and B (129) takes its slot while A is in window 1; C closes after one
    window and D (64) takes its slot -> {name: joined output}.  Checks on the way that the slots are reused as said."""
    acc = {k: [] for k in "ABCDE"}
    a, c, e = sb.open(), sb.open(), sb.open()
    assert (a.slot, c.slot, e.slot) == (0, 1, 2)
    feed_window(a, w["A"], chunk), feed(c, w["C"], len(w["C"]), chunk), feed(e, w["E"], len(w["E"]), chunk)
    acc["E"].append(e.close())                                                     # a recording that is only a tail: everything in close()
    out = sb.step()
    assert set(out) == {a, c} and a.windows == 1
    acc["A"].append(out[a]), acc["C"].append(out[c])
    b = sb.open()
    assert b.slot == 2
    feed_window(b, w["B"], chunk), feed_window(a, w["A"], chunk)
    acc["C"].append(c.close())
    d = sb.open()
    assert d.slot == 1
    feed(d, w["D"], len(w["D"]), chunk)
    out = sb.step()                                                                # A in window 1, B and D in window 0
    assert set(out) == {a, b, d}
    acc["A"].append(out[a]), acc["B"].append(out[b]), acc["D"].append(out[d])
    acc["D"].append(d.close())
    while True:
        feed_window(a, w["A"], chunk), feed_window(b, w["B"], chunk)
        out = sb.step()
        if not out:
            break
        for s, name in ((a, "A"), (b, "B")):
            if s in out:
                acc[name].append(out[s])
    acc["A"].append(a.close()), acc["B"].append(b.close())
    assert (a.windows, b.windows, c.windows, d.windows, e.windows) == (5, 2, 1, 1, 0)
    return {k: joined(v) for k, v in acc.items()}


def check_against_golden(name, got, golden_dir, label=""):
    """Code indices identical to the reference's B = 1 golden of the same waveform, arrays within TOL, the golden's shapes."""
    g = np.load(os.path.join(golden_dir, f"infer_{FRAMES[name]}f_b1.npz"))
    poses, expressions, trans, codes = got
    n = FRAMES_OUT[name]
    assert poses.shape == (n, 165) and expressions.shape == (n, 100) and trans.shape == (n, 3) and g["poses"].shape == (1, n, 165)
    for p in PARTS:
        assert np.array_equal(codes[p], g[f"index_{p}"][0]), f"{name}: {p} code indices differ"
    for nm, x in (("poses", poses), ("expressions", expressions), ("trans", trans)):
        err = float(np.abs(x - g[nm][0]).max())
        print(f"{label} {name} ({FRAMES[name]}f) {nm}: max|err| {err:.2e}")
        assert err < TOL, (name, nm, err)
