#!/usr/bin/env python
"""What one validation step (train_emage_audio.py:130-204, mode="val") costs on the MI355X at 56 clips of 64 frames, three ways:
  eager_parent   the composition a user could write before `validation.Validator` existed: three eval `model(...)` calls (each runs both
                 WavEncoders again), `training.losses` for each (24 loss launches), `model._select_codes` (`ops.argmax_logsoftmax`),
                 `vq.decode`, and the six losses read back on the host;
  step           `Validator.step`: the shared WavEncoder pass, one `ops.val_metrics` call, one read-back at the end;
  replay         `Validator.capture` + `replay()`: the same step as one hipGraph, nothing read back.
Wall time per step around a run that ends in a device synchronise; the three arms alternate, `--runs` times each, and the run-to-run spread
is reported.  `emage_op_calls`: calls into libemage_hip.so per step — a replay issues those of `step`, plus `replay_repack_extra` for the
packing graph when the parameters have changed since the last replay (never inside the timed runs here; `replay_repack` times a replay
that is forced to pack); torch's own small kernels are not in that count.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


class CallCounter:
    """The measurement hook of `ops` (`_TRACE`): counts the operator calls that reach the library."""

    def __init__(self):
        self.calls = 0

    def tag(self):
        return None

    def fire(self, kind, entries, launch):
        self.calls += 1
        return launch()


def counted(fn):
    from pantomatrix_amd import ops
    counter = CallCounter()
    ops._TRACE[0] = counter
    try:
        fn()
    finally:
        ops._TRACE[0] = None
    return counter.calls


def summary(values):
    return {"runs": [round(v, 3) for v in values], "median": round(float(np.median(values)), 3), "spread": round(max(values) - min(values), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=56)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed run")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--commit", default=None, help="recorded in the line (the measured tree is not always a git checkout)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_validation needs an MI355X: none of its figures means anything on a CPU"
    from pantomatrix_amd import data, ops, training, validation
    from tools import workloads
    dev = "cuda"
    b, t = args.batch, args.frames
    model, vq = workloads.product_models(precision=args.precision, device=dev)
    cfg = model.config
    batch = {k: v.to(dev) for k, v in workloads.train_batch(bs=b, t=t).items()}
    mask = (torch.rand(b, t, data.MASK_DIMS, generator=torch.Generator().manual_seed(6)) < 0.05).float().to(dev)

    def eager_parent():
        index, latent, masked_motion = training.targets(vq, batch["motion"], batch["expressions"], batch["trans"], batch["foot_contact"])
        speaker_id = torch.zeros(b, 1, dtype=torch.long, device=dev)
        seed_mask = torch.ones_like(masked_motion)
        seed_mask[:, :cfg.seed_frames] = 0
        ws = ops.loss_workspace(dev)
        out, first = {}, None
        for tag, m, use_audio in (("seed", seed_mask, True), ("audio", mask, True), ("mask", mask, False)):
            pred = model(batch["audio"], speaker_id, masked_motion, m, use_audio=use_audio)
            first = pred if first is None else first
            out["rec_" + tag], out["cls_" + tag] = training.losses(cfg, pred, index, latent, ws)
        dec = vq.decode(**model._select_codes(first))["all_motion4inference"][:, :, :-7]
        res = {k: float(v) for k, v in out.items()}
        ops.loss_check(ws)
        return res, dec

    val = validation.Validator(model, vq)
    graph_val = validation.Validator(model, vq)
    calls = {"eager_parent": None, "step": None, "replay": None}
    ref, _dec = eager_parent()                                # warm-up of every shape, and the numbers the arms must agree on
    got = val.step(batch, mask)
    calls["eager_parent"] = counted(eager_parent)
    calls["step"] = counted(lambda: val.step(batch, mask))
    captured = counted(lambda: graph_val.capture(batch, mask))                  # one warm-up step, the packing graph, the step's graph
    calls["replay"], calls["replay_repack_extra"] = calls["step"], captured - 2 * calls["step"]
    graph_val.reset()
    graph_val.replay()
    replayed = graph_val.result()
    for k, v in ref.items():
        assert abs(got[k] - v) < 2e-4 * max(1.0, abs(v)) and abs(replayed[k] - v) < 2e-4 * max(1.0, abs(v)), (k, v, got[k], replayed[k])
    arms = {"eager_parent": eager_parent, "step": lambda: val.step(batch, mask), "replay": graph_val.replay,
            "replay_repack": lambda: graph_val.replay(repack=True)}
    ms = {k: [] for k in arms}
    torch.cuda.synchronize()
    for _ in range(args.runs):
        for name, fn in arms.items():
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - t0) / args.steps)
    line = {"what": "one validation step (three eval forwards, losses, codes, accuracies, decode): eager composition of the parent commit vs Validator.step vs replay()",
            "commit": args.commit, "config": {"clips": b, "frames_per_clip": t, "precision": args.precision, "steps_per_run": args.steps},
            "ms_per_step": {k: summary(v) for k, v in ms.items()}, "emage_op_calls": calls,
            "losses": {k: round(v, 6) for k, v in got.items() if not k.startswith("acc_")},
            "replay_over_eager_parent": round(float(np.median(ms["replay"]) / np.median(ms["eager_parent"])), 3),
            "peak_memory_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
