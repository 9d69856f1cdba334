"""The workloads whose op sequence tests/golden/call_logs.json pins (tests/golden/make_call_logs.py records it, test_window_step_host.py
compares): every `ops` entry point the CPU stand-ins log into `fake_ops.CALLS`, in order, for
  (a) `infer_codes` at 70 and 129 frames, B = 2;
  (b) an eager `RecordingRunner` pass over the recordings of 70 / 310 / 40 / 129 / 64 frames: plain, with max_batch = 2 and per-recording
      speaker ids, and hinted with tests/golden/infer_hints_*.npz;
  (c) the five-session scenario of tests/test_stream_host.py, ticks and closes.
The op sequence is the launch sequence, and so what a captured graph holds.  Construction (a runner's warm-up pass included) is not
logged: only the pass / the scenario itself."""
import hashlib
import os

import numpy as np
import torch

import common
import fake_hint_ops
import fake_ops
import fake_stream_ops
import speaker_common
import stream_common as sc
from pantomatrix_amd import recordings as R, streaming, synthetic

FRAMES = (70, 310, 40, 129, 64)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _wave(frames, batch=1):
    return synthetic.synthetic_audio(batch, synthetic.samples_for_frames(frames), seed=1234)


def _logged(fn):
    fake_ops.CALLS.clear()
    fn()
    return list(fake_ops.CALLS)


def _infer_codes(frames):
    model, vq = common.product_models(precision="fp32")
    model.infer_codes(_wave(9, 2), torch.zeros(2, 1, dtype=torch.long), vq)         # packs the operand sets: not part of the log
    return _logged(lambda: model.infer_codes(_wave(frames, 2), torch.zeros(2, 1, dtype=torch.long), vq))


def _recordings(speaker_ids=None, hinted=False, **kw):
    model, vq = common.product_models(precision="fp32") if speaker_ids is None else speaker_common.product_models(3)
    motions = masks = None
    if hinted:
        files = [np.load(os.path.join(GOLDEN, f"infer_hints_{f}f_b1.npz")) for f in FRAMES]
        motions = [g["hint_motion"] if bool(g["has_motion"]) else None for g in files]
        masks = [g["hint_keep"] if bool(g["has_mask"]) else None for g in files]
    rs = R.RecordingSet.from_audio([_wave(f)[0] for f in FRAMES], "cpu", speaker_ids=speaker_ids, masked_motion=motions, mask=masks)
    runner = R.RecordingRunner.for_set(model, vq, rs, use_graph=False, **kw)
    return _logged(lambda: runner(rs))


def _stream():
    sb = streaming.StreamBatch(*common.product_models(precision="fp32"), slots=3, max_seconds=11, use_graph=False)
    return _logged(lambda: sc.scenario(sb, sc.waves()))


WORKLOADS = {
    "infer_codes_70f_b2": lambda: _infer_codes(70),
    "infer_codes_129f_b2": lambda: _infer_codes(129),
    "recordings_plain": _recordings,
    "recordings_ids_max_batch_2": lambda: _recordings(speaker_ids=[0, 1, 2, 1, 0], max_batch=2),
    "recordings_hinted": lambda: _recordings(hinted=True),
    "stream_five_sessions": _stream,
}


def calls_of(name):
    """-> [op names in call order] of one workload, over the CPU stand-ins of every kernel."""
    with fake_hint_ops.installed(), fake_stream_ops.installed(), torch.no_grad():
        return WORKLOADS[name]()


def digest(calls):
    """What the fixture keeps of one call list: its length, the count per name and a SHA-256 of the newline-joined names."""
    counts = {}
    for c in calls:
        counts[c] = counts.get(c, 0) + 1
    return {"n": len(calls), "sha256": hashlib.sha256("\n".join(calls).encode()).hexdigest(), "counts": dict(sorted(counts.items()))}
