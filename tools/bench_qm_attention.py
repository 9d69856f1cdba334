#!/usr/bin/env python
"""A/B of `compose_memory` and of the stack sites that compute their own K / V^T (ops.qm_attention, csrc/q_attention.hip) in the flagship step
(bench.py's: ClipRunner graph replay of 64 clips x 128 frames, f16x3).  Three forms of the same step:

  plain     compose_memory off: the memory projections, the plain K / V launches (K = 768), the q sites — the step before this change;
  composed  compose_memory on, fuse_memory_kv off: one composed K / V launch per stack (K = 256 / 512), the q sites;
  site      both on (the default): no K / V launch, every stack site computes its own.

  --step:     the three forms interleaved in ONE process, `--pairs` rounds of `--steps` replays each (the order rotates); prints every round,
              and per comparison the mean gain, its standard deviation over the rounds and whether every round gains;
  --one FORM: `--steps` replays of the serialized step (every chain on one stream) of one form — the run
              `rocprofv3 --kernel-trace --stats -- python tools/bench_qm_attention.py --one site` profiles.
Usage: python tools/bench_qm_attention.py [--step] [--pairs 8] [--steps 100] [--one plain|composed|site]"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

DEV = "cuda"
FORMS = {"plain": (False, False), "composed": (True, False), "site": (True, True)}


def _models(form):
    from tools import workloads as common
    from pantomatrix_amd import synthetic
    b, n = 64, synthetic.samples_for_frames(128)
    audio = synthetic.synthetic_audio(b, n).to(DEV)
    model, vq = common.product_models(precision="f16x3", device=DEV)
    model.compose_memory, model.fuse_memory_kv = FORMS[form]
    return model, vq, audio, b, n


def step(pairs, steps, warmup):
    from pantomatrix_amd.runtime import ClipRunner
    runners = {}
    for form in FORMS:                                   # a model per form: each keeps its own packed set and captured graph
        model, vq, audio, b, n = _models(form)
        runners[form] = ClipRunner(model, vq, b, n, use_graph=True)
        for _ in range(warmup):
            runners[form](audio)
    torch.cuda.synchronize()

    def ms(form):
        r = runners[form]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            r(audio)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps

    names = list(FORMS)
    rows = []
    for i in range(pairs):
        order = names[i % 3:] + names[:i % 3]
        got = {f: ms(f) for f in order}
        rows.append(got)
        print(json.dumps({"round": i, **{f + "_ms": got[f] for f in names}}), flush=True)
    for slow, fast in (("plain", "site"), ("plain", "composed"), ("composed", "site")):
        gains = [r[slow] - r[fast] for r in rows]
        mean = sum(gains) / len(gains)
        sd = math.sqrt(sum((g - mean) ** 2 for g in gains) / max(1, len(gains) - 1))
        print(json.dumps({f"{fast}_vs_{slow}": {"rounds": len(rows), "mean_gain_ms": mean, "sd_ms": sd, "every_round_gains": all(g > 0 for g in gains),
                                                 f"{slow}_ms_mean": sum(r[slow] for r in rows) / len(rows),
                                                 f"{fast}_ms_mean": sum(r[fast] for r in rows) / len(rows)}}), flush=True)


def one_form(form, steps):
    from pantomatrix_amd.runtime import ClipRunner
    model, vq, audio, b, n = _models(form)
    for p in (model, vq.vq_model_face, vq.vq_model_upper, vq.vq_model_hands, vq.vq_model_lower, vq.global_motion):
        p.concurrent = False
    r = ClipRunner(model, vq, b, n, use_graph=True)
    for _ in range(steps):
        r(audio)
    torch.cuda.synchronize()
    print(json.dumps({"form": form, "steps": steps}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--one", choices=tuple(FORMS), default=None, help="serialized steps of ONE form (profiling runs)")
    args = ap.parse_args()
    with torch.no_grad():
        if args.one is not None:
            one_form(args.one, args.steps)
        elif args.step:
            step(args.pairs, args.steps, args.warmup)
