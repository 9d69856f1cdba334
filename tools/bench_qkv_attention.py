#!/usr/bin/env python
"""A/B of the fused self-attention site (ops.qkv_attention, csrc/qkv_attention.hip) against the two launches it replaces.

  --kernels: per-launch device time at the flagship shape (64 clips x 64 frames, d = 768, LayerNorm fold on): the qkv projection
             (emage_gemm: q / k float32 + V^T), emage_attention on its output, and the fused launch (HIP events around `--reps` launches);
  --step:    the flagship step (bench.py's: ClipRunner graph replay of 64 clips x 128 frames, f16x3) with `fuse_self_attention` on and off,
             interleaved in ONE process, `--pairs` pairs of `--steps` replays each; prints every pair and the mean gain.
  --one 0|1: `--steps` replays of the serialized step (every chain on one stream) with the fused sites off / on, and the peak of allocated
             device memory — the run `rocprofv3 --kernel-trace --stats -- python tools/bench_qkv_attention.py --one 1` profiles.
Usage: python tools/bench_qkv_attention.py [--kernels] [--step] [--pairs 4] [--steps 50] [--one 0|1]"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from pantomatrix_amd import ops  # noqa: E402

DEV = "cuda"


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def kernels(reps):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_qkv_attention_gpu import _site, D, T, H
    b = 64
    dt, a, w, bias, w_s, ln = _site(b, True, 0, seed=5)
    m = b * T
    qk, vt = torch.zeros(m, 2 * D, device=DEV), torch.zeros(b, D, T, device=DEV)
    att, att2 = torch.zeros(m, D, device=DEV), torch.zeros(m, D, device=DEV)
    proj = lambda: ops.gemm(dt, a, w, bias, None, None, None, qk, vt, n=3 * D, cp=D, w_scale=w_s, t_col0=2 * D, t_rows=T, ln=ln)
    attn = lambda: ops.attention(dt, qk[:, :D], qk[:, D:], vt, D, att, b, H, T, T, D // H)
    fused = lambda: ops.qkv_attention(dt, a, w, bias, att2, b, w_scale=w_s, ln=ln)
    res = {}
    for _ in range(2):                                   # interleaved rounds: the second one is reported
        res = {"qkv_projection_us": _time(proj, reps), "attention_us": _time(attn, reps), "fused_us": _time(fused, reps)}
    res["two_launches_us"] = res["qkv_projection_us"] + res["attention_us"]
    res["same_bits"] = bool(torch.equal(att.view(torch.int32), att2.view(torch.int32)))
    print(json.dumps({"kernels": res}))


def step(pairs, steps, warmup):
    from tools import workloads as common
    from pantomatrix_amd import synthetic
    from pantomatrix_amd.runtime import ClipRunner
    b = 64
    n = synthetic.samples_for_frames(128)
    audio = synthetic.synthetic_audio(b, n).to(DEV)
    model, vq = common.product_models(precision="f16x3", device=DEV)
    runners = {}
    for fuse in (True, False):
        model.fuse_self_attention = fuse
        runners[fuse] = ClipRunner(model, vq, b, n, use_graph=True)
        for _ in range(warmup):
            runners[fuse](audio)
    torch.cuda.synchronize()

    def ms(fuse):
        r = runners[fuse]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            r(audio)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps

    rows = []
    for i in range(pairs):
        order = (True, False) if i % 2 == 0 else (False, True)
        got = {f: ms(f) for f in order}
        rows.append({"on_ms": got[True], "off_ms": got[False], "gain_ms": got[False] - got[True]})
        print(json.dumps({"pair": i, **rows[-1]}), flush=True)
    gains = [r["gain_ms"] for r in rows]
    mean = sum(gains) / len(gains)
    sd = math.sqrt(sum((g - mean) ** 2 for g in gains) / max(1, len(gains) - 1))
    print(json.dumps({"step": {"pairs": len(rows), "mean_gain_ms": mean, "sd_ms": sd, "every_pair_gains": all(g > 0 for g in gains),
                               "on_ms_mean": sum(r["on_ms"] for r in rows) / len(rows), "off_ms_mean": sum(r["off_ms"] for r in rows) / len(rows)}}))


def one_config(fuse, steps):
    """A fresh process per setting: `steps` graph replays of the flagship step with every launch chain on ONE stream (the serialized step:
    what `rocprofv3 --kernel-trace --stats` is run over), then the peak of allocated device memory."""
    from tools import workloads as common
    from pantomatrix_amd import synthetic
    from pantomatrix_amd.runtime import ClipRunner
    b = 64
    n = synthetic.samples_for_frames(128)
    audio = synthetic.synthetic_audio(b, n).to(DEV)
    model, vq = common.product_models(precision="f16x3", device=DEV)
    model.fuse_self_attention = fuse
    for p in (model, vq.vq_model_face, vq.vq_model_upper, vq.vq_model_hands, vq.vq_model_lower, vq.global_motion):
        p.concurrent = False
    torch.cuda.reset_peak_memory_stats()
    r = ClipRunner(model, vq, b, n, use_graph=True)
    for _ in range(steps):
        r(audio)
    torch.cuda.synchronize()
    print(json.dumps({"fuse": fuse, "steps": steps, "peak_allocated_mb": torch.cuda.max_memory_allocated() / 2 ** 20}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--one", type=int, choices=(0, 1), default=None, help="serialized steps + peak memory of ONE setting (profiling runs)")
    args = ap.parse_args()
    if args.one is not None:
        with torch.no_grad():
            one_config(bool(args.one), args.steps)
        sys.exit(0)
    with torch.no_grad():
        if args.kernels:
            kernels(args.reps)
        if args.step:
            step(args.pairs, args.steps, args.warmup)
