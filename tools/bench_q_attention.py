#!/usr/bin/env python
"""A/B of the fused cross-attention site (ops.q_attention, csrc/q_attention.hip) against the two launches it replaces.

  --kernels: per-launch device time at the flagship shape (64 clips x 64 frames, d = 768, LayerNorm fold on, K / V^T one layer of an 8-layer
             memory): the q projection (emage_gemm: q float32), emage_attention on it, the two back to back, and the fused launch — each as a
             captured graph of `--reps` launches, replayed `--rounds` times interleaved (min / median / max per form);
  --step:    the flagship step (bench.py's: ClipRunner graph replay of 64 clips x 128 frames, f16x3) with `fuse_cross_attention` on and off,
             interleaved in ONE process, `--pairs` pairs of `--steps` replays each; prints every pair and the mean gain;
  --one 0|1: `--steps` replays of the serialized step (every chain on one stream) with the fused sites off / on — the run
             `rocprofv3 --kernel-trace --stats -- python tools/bench_q_attention.py --one 1` profiles.
Usage: python tools/bench_q_attention.py [--kernels] [--step] [--pairs 4] [--steps 50] [--one 0|1]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from pantomatrix_amd import ops  # noqa: E402

DEV = "cuda"


def _graph_of(fn, reps):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def _replay_us(g, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def site(b=64, layers=8, layer=3, seed=5):
    """The flagship site's operands: a folded operand as tests/test_qkv_attention_gpu.py builds it (the q third of its packed projection)
    and layer `layer` of a `layers`-layer memory."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_qkv_attention_gpu import _site, D, T, H
    dt, a, w, bias, w_s, ln = _site(b, True, 0, seed=seed)
    g = torch.Generator().manual_seed(seed)
    kbuf = torch.randn(b * T, layers * D, generator=g).to(DEV)
    vtbuf = torch.randn(b, layers * D, T, generator=g).to(DEV)
    return dict(dt=dt, a=a, w=w[:D].contiguous(), bias=bias[:D].contiguous(), w_s=w_s, ln=(ln[0], ln[1][:D].contiguous()),
                k=kbuf[:, layer * D:(layer + 1) * D], vt=vtbuf[:, layer * D:], vt_rows=layers * D, b=b, D=D, T=T, H=H)


def kernels(reps, rounds, s=None, label="kernels"):
    s = site() if s is None else s
    b, D, T, H, dt = s["b"], s["D"], s["T"], s["H"], s["dt"]
    m = b * T
    q, att, att2 = torch.zeros(m, D, device=DEV), torch.zeros(m, D, device=DEV), torch.zeros(m, D, device=DEV)
    proj = lambda: ops.gemm(dt, s["a"], s["w"], s["bias"], None, None, None, q, None, n=D, cp=D, w_scale=s["w_s"], ln=s["ln"])
    attn = lambda: ops.attention(dt, q, s["k"], s["vt"], s["vt_rows"], att, b, H, T, T, D // H)
    fused = lambda: ops.q_attention(dt, s["a"], s["w"], s["bias"], s["k"], s["vt"], s["vt_rows"], att2, b, w_scale=s["w_s"], ln=s["ln"])

    def both():
        proj()
        attn()

    forms = {"q_projection_us": proj, "attention_us": attn, "two_launches_us": both, "fused_us": fused}
    graphs = {k: _graph_of(f, reps) for k, f in forms.items()}
    times = {k: [] for k in forms}
    for _ in range(rounds):                              # interleaved rounds
        for k, g in graphs.items():
            times[k].append(_replay_us(g, reps))
    res = {k: {"min": min(v), "median": statistics.median(v), "max": max(v)} for k, v in times.items()}
    gains = [t - f for t, f in zip(times["two_launches_us"], times["fused_us"])]
    res["gain_us"] = {"min": min(gains), "median": statistics.median(gains), "max": max(gains)}
    res["same_bits"] = bool(torch.equal(att.view(torch.int32), att2.view(torch.int32)))
    print(json.dumps({label: res}), flush=True)
    return res


def _runner(model, vq, audio, b, n):
    from pantomatrix_amd.runtime import ClipRunner
    return ClipRunner(model, vq, b, n, use_graph=True)


def step(pairs, steps, warmup):
    from tools import workloads as common
    from pantomatrix_amd import synthetic
    b = 64
    n = synthetic.samples_for_frames(128)
    audio = synthetic.synthetic_audio(b, n).to(DEV)
    model, vq = common.product_models(precision="f16x3", device=DEV)
    runners = {}
    for fuse in (True, False):
        model.fuse_cross_attention = fuse
        runners[fuse] = _runner(model, vq, audio, b, n)
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
    what `rocprofv3 --kernel-trace --stats` is run over)."""
    from tools import workloads as common
    from pantomatrix_amd import synthetic
    b = 64
    n = synthetic.samples_for_frames(128)
    audio = synthetic.synthetic_audio(b, n).to(DEV)
    model, vq = common.product_models(precision="f16x3", device=DEV)
    model.fuse_cross_attention = fuse
    for p in (model, vq.vq_model_face, vq.vq_model_upper, vq.vq_model_hands, vq.vq_model_lower, vq.global_motion):
        p.concurrent = False
    r = _runner(model, vq, audio, b, n)
    for _ in range(steps):
        r(audio)
    torch.cuda.synchronize()
    print(json.dumps({"fuse_cross_attention": fuse, "steps": steps}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--one", type=int, choices=(0, 1), default=None, help="serialized steps of ONE setting (profiling runs)")
    args = ap.parse_args()
    if args.one is not None:
        with torch.no_grad():
            one_config(bool(args.one), args.steps)
        sys.exit(0)
    with torch.no_grad():
        if args.kernels:
            kernels(args.reps, args.rounds)
        if args.step:
            step(args.pairs, args.steps, args.warmup)
