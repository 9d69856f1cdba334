#!/usr/bin/env python
"""bench.py — EMAGE inference throughput on MI355X (BASELINE.json metric: motion-frames/s, 128-frame clips).

One "step" = one pass of the hot path over one batch of 64 synthetic 128-frame clips per GPU:
`EmageAudioModel.inference` (2 dependent 64-frame windows) + the final `EmageVQModel.decode(get_global_motion=
True)` + D2H of poses/expressions/trans, audio already resident in HBM (the PCIe-inclusive rate is measured beside it
and reported as `pcie_inclusive`, never as `value`).  120 frames are emitted per clip.

Precision: `f16x3` (default) is the parity-green mode — float32 storage, every contraction as three split-fp16 MFMAs
with fp32 accumulate: VQ code indices identical to the reference on every golden clip incl. the 64-clip batch, SMPL-X
parameters within 1e-3 (tests/test_parity_gpu.py).  The pure-bf16 mode (not index-exact) is timed beside it and
reported under `other_precisions`.

N > 1: one process per GPU; `python bench.py --gpus N` without a launcher re-executes itself under
torch.distributed.run (127.0.0.1 rendezvous).  Clips are sharded across ranks, no data-path collective ("replicas
only", weak scaling); RCCL carries the barriers and the max-over-ranks of the timing only.

Prints ONE JSON line on rank 0 with the contract fields.  A plain run does only what that line needs: set-up, warm-up, the
timed steps and, with `--dump-outputs DIR`, the last timed step's results (poses, expressions, trans) as DIR/<name>.npy.
`--full` adds everything else the benchmark measures: `pcie_inclusive`, `roofline` (dominant kernel family; every kernel
of one serialized step timed live with HIP events on the launch stream), `code_agreement`, `other_precisions`,
`cpu_baseline` (the CPU oracle, a port of the reference, timed on this host on a bounded sample), `config1`,
`batch_sweep`, `lstm_models` and `train_step`.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

F16_MFMA_PEAK_TFLOPS = 2500.0    # dense bf16 / fp16 MFMA, MI355X_MICROARCH.md
F32_MFMA_PEAK_TFLOPS = 157.3
HBM_PEAK_GBS = 8000.0
METRIC = "motion-frames/sec (30fps SMPL-X) EMAGE infer, 128-frame clips"
PRECISION_NOTE = {
    "f16x3": "4-byte storage (float32; contraction operands pre-split by their producers into fp16 hi | lo images), each product as 3 split-fp16 MFMAs (hi*hi + hi*lo + lo*hi), fp32 accumulate: parity-green "
             "(bit-exact VQ indices, 1e-3 rotations vs the reference)",
    "bf16": "bf16 operands, fp32 accumulate: NOT index-exact (about 97.5 % of frames keep all body codes)",
    "fp32": "exact-fp32 MFMA (v_mfma_f32_16x16x4_f32): parity-green, slow",
}


def usable_cores():
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return max(1, n)


def log(msg):
    print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


class native_stdout_to_stderr:
    """Context: file descriptor 1 points at stderr while native libraries initialise — RCCL prints a version banner ("RCCL version : ...",
    "Librccl path : ...") to the C-level stdout when its first communicator is created, which would put extra lines next to the ONE JSON line
    the contract promises on stdout.  C stdio is flushed on both edges, so nothing written inside can surface later on the real stdout."""

    def __enter__(self):
        import ctypes
        self._libc = ctypes.CDLL(None)
        sys.stdout.flush()
        self._libc.fflush(None)
        self._saved = os.dup(1)
        os.dup2(2, 1)
        return self

    def __exit__(self, *exc):
        sys.stdout.flush()
        self._libc.fflush(None)
        os.dup2(self._saved, 1)
        os.close(self._saved)
        return False


# ----------------------------------------------------------------------------------------------------------------------
# multi-GPU launch: one process per GPU
# ----------------------------------------------------------------------------------------------------------------------
def spawn_command(argv, n_gpus, port):
    """The command `python bench.py --gpus N` re-executes when no launcher set WORLD_SIZE: the driver's own recipe."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_gpus}",
            "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)


def free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def timed_steps(step, steps, warmup, barrier, reduce_max):
    """The contract's timed region: `warmup` untimed steps, then exactly `steps` steps bracketed by a barrier +
    device synchronisation on both sides; returns (max-over-ranks seconds, last step's result)."""
    out = None
    for _ in range(warmup):
        out = step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = step()
    barrier()
    return reduce_max(time.perf_counter() - t0), out


def timed_pipeline(pipe, audio, steps, warmup, barrier, reduce_max):
    """The same timed region with `pipe.depth` batches in flight (runtime.ClipPipeline): exactly `steps` batches are submitted
    AND collected (results on the host, health-checked) between the two barriers."""
    for _ in range(warmup):
        pipe.submit(audio)
    pipe.drain()
    barrier()
    t0 = time.perf_counter()
    out = None
    for _ in range(steps):
        r = pipe.submit(audio)
        out = r if r is not None else out
    rest = pipe.drain()
    out = rest[-1] if rest else out
    barrier()
    return reduce_max(time.perf_counter() - t0), out


OUTPUT_NAMES = ("poses", "expressions", "trans")       # what ClipRunner.__call__ hands its caller, in its order
DUMP_BUDGET_BYTES = 64 << 20


def dump_outputs(directory, outputs):
    """Write the arrays of the last timed step as DIR/<name>.npy (float32), for output-for-output comparison of two builds.  A batch
    whose arrays exceed 64 MB in all is cut to its first clips (the same clips in every run with the same arguments)."""
    arrays = [np.asarray(a, dtype=np.float32) for a in outputs]
    per_clip = sum(a[:1].nbytes for a in arrays)
    clips = min(len(arrays[0]), DUMP_BUDGET_BYTES // per_clip)
    os.makedirs(directory, exist_ok=True)
    for name, a in zip(OUTPUT_NAMES, arrays):
        np.save(os.path.join(directory, name + ".npy"), np.ascontiguousarray(a[:clips]))
    log(f"outputs of the last timed step ({clips} of {len(arrays[0])} clips) written to {directory}")


def result_line(precision, elapsed, steps, warmup, world, frames_per_step, batch, frames_in, launch):
    return {
        "metric": METRIC,
        "value": frames_per_step * world * steps / elapsed,
        "unit": "motion-frames/s",
        "n_gpus": world, "steps": steps, "warmup": warmup,
        "ms_per_step": 1e3 * elapsed / steps,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": precision, "data": "synthetic",
        "config": {"workload": f"EMAGE inference {precision}, batch={batch}x{frames_in}-frame synthetic clips per GPU "
                               f"(BASELINE configs[1]): 2 windows of 64 frames + final VQ decode with global motion, "
                               f"{frames_per_step // batch} frames out per clip; synthetic seeded weights",
                   "precision": PRECISION_NOTE[precision],
                   "clips_per_gpu": batch, "frames_in": frames_in, "frames_out_per_clip": frames_per_step // batch,
                   "parallelism": f"replicas x{world} (clip-sharded, no collective)", "launch": launch},
    }


# ----------------------------------------------------------------------------------------------------------------------
# live per-kernel timing of one serialized step
# ----------------------------------------------------------------------------------------------------------------------
def profile_kernels(runner, model, vq):
    """One extra, untimed pass of the SAME launch sequence the timed graph replays (`ClipRunner._step`: the lean code
    path), issued eagerly on ONE stream (no fork / join lanes) with a HIP-event pair around every kernel launch on that
    stream — through the op layer's measurement hook (`ops._TRACE`), which brackets every ACTUAL launch: single ops and the
    grouped contractions of the lock-step chains (`emage_gemm_grouped`: one record per library launch, flops = the sum over its problems).
    A backlog of filler GEMMs is enqueued first so that the host runs ahead of the device: each event pair then
    brackets exactly one kernel's device time (plus the event markers), not host launch latency.
    Returns (records, marker_ms): records = [(tag, scope, ms, flops, bytes)]."""
    from pantomatrix_amd import ops, modeling_emage_audio as M
    from pantomatrix_amd._lib import BF16
    records, scope = [], {"name": None}

    def gemm_cost(a, meta):
        dtype, A, n, cp, taps, m = a[0], a[1], a[9], a[10], a[15], a[20]
        es = 2 if dtype == BF16 else 4
        kk = meta.get("k_real") or taps * cp                 # unpadded contraction length
        io = sum(t.numel() * t.element_size() for t in a[5:9] if torch.is_tensor(t))      # residual read + every output written
        return ("emage_gemm", 2.0 * m * n * kk, float(m * cp * es + n * taps * cp * es + io))

    def attn_cost(a, meta):
        dtype, b, h, tq, tk, hd = a[0], a[6], a[7], a[8], a[9], a[10]
        es = 2 if dtype == BF16 else 4
        return ("emage_attention", 4.0 * b * h * tq * tk * hd, float((2 * b * tq + 2 * b * tk) * h * hd * es))

    def vq_cost(a, meta):
        z, cb = a[0], a[1]
        n, d = z.shape
        return ("emage_vq_argmin", 2.0 * n * cb.shape[0] * d, float(n * d * 4 + cb.shape[0] * d * 4 + n * 8))

    def generic_cost(tag):
        def c(a, meta):
            return ("emage_" + tag, 0.0, float(sum(t.numel() * t.element_size() for t in a if torch.is_tensor(t))))
        return c

    def slab_cost(a, meta):
        dtype, W, nseq, l, taps = a[0], a[2], a[7], a[8], a[9]
        c = W.shape[0]
        rows = nseq * l
        es = 2 if dtype == BF16 else 4
        return ("emage_conv_slab", 2.0 * rows * c * taps * c, float(2 * rows * c * es + c * taps * c * es))

    def block0_cost(a, meta):
        dtype, wav, w1, taps2, out = a[0], a[1], a[2], a[12], a[14]
        c, t1 = w1.shape
        rows = out.shape[0]
        es = 2 if dtype == BF16 else 4
        return ("emage_conv_slab", 2.0 * rows * c * taps2 * c + 2.0 * rows * 2 * c * t1, float(wav.numel() * 4 + rows * c * es))

    table = {"gemm": gemm_cost, "attention": attn_cost, "vq_argmin": vq_cost, "conv_slab": slab_cost, "wav_block0": block0_cost}

    def cost_of(entry):
        name, _op, a, meta = entry
        return table.get(name, generic_cost(name))(a, meta)

    class Tracer:
        def tag(self):
            return scope["name"]

        def fire(self, kind, entries, launch):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = launch()
            e1.record()
            costs = [cost_of(e) for e in entries]
            tags = {e[3].get("tag") for e in entries}
            sc = tags.pop() if len(tags) == 1 else None
            launches = ops.grouped_launch_count(entries) if kind == "gemm_grouped" else 1
            # a grouped call that the library splits into several launches is booked as that many equal records
            for _ in range(launches):
                records.append((e0 if _ == 0 else None, e1 if _ == 0 else None, sc, costs[0][0], sum(c[1] for c in costs) / launches,
                                sum(c[2] for c in costs) / launches, launches))
            return r

    def scoped(fn, name):
        def inner(*a, **k):
            prev, scope["name"] = scope["name"], name
            try:
                return fn(*a, **k)
            finally:
                scope["name"] = prev
        return inner

    parts = [model, vq.vq_model_face, vq.vq_model_upper, vq.vq_model_hands, vq.vq_model_lower, vq.global_motion]
    concurrent = [p.concurrent for p in parts]
    layer_fns = {nm: getattr(M.EmageAudioModel, nm) for nm in ("_decoder_layer", "_encoder_layer", "_memory_kv")}
    try:
        for nm, fn in layer_fns.items():                    # the 16 transformer layers incl. their memory K/V projections
            setattr(M.EmageAudioModel, nm, scoped(fn, "transformer_blocks"))
        for p in parts:
            p.concurrent = False
        filler_a = torch.randn(8192, 8192, device=model.device, dtype=torch.bfloat16)
        filler_o = torch.empty(8192, 8192, device=model.device, dtype=torch.bfloat16)
        torch.cuda.synchronize()
        for _ in range(40):                                 # ~1.1 TFLOP each: tens of ms of device backlog (this library's own bf16 GEMM: no vendor kernel in the process)
            ops.gemm(BF16, filler_a, filler_a, None, None, None, filler_o, None, None, n=8192, cp=8192)
        ops._TRACE[0] = Tracer()
        empties = []                                        # event pairs with nothing between them: the markers' own cost
        for _ in range(64):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            e1.record()
            empties.append((e0, e1))
        runner._step()
        torch.cuda.synchronize()
        marker_ms = float(np.median([a.elapsed_time(b) for a, b in empties]))
    finally:
        ops._TRACE[0] = None
        for nm, fn in layer_fns.items():
            setattr(M.EmageAudioModel, nm, fn)
        for p, c in zip(parts, concurrent):
            p.concurrent = c
    out, last_ms = [], 0.0
    for e0, e1, sc, tag, flops, byts, launches in records:
        if e0 is not None:
            last_ms = e0.elapsed_time(e1) / launches
        out.append((tag, sc, last_ms, flops, byts))
    return out, marker_ms


def serialized_graph_ms(model, vq, args, n_samples, audio, steps):
    """Wall time per step of the SAME launch sequence captured as a single-stream hipGraph (no fork / join lanes): with
    nothing to overlap, this is the sum of the kernels' device times (rocprofv3 of that graph shows no gaps)."""
    from pantomatrix_amd.runtime import ClipRunner
    parts = [model, vq.vq_model_face, vq.vq_model_upper, vq.vq_model_hands, vq.vq_model_lower, vq.global_motion]
    saved = [p.concurrent for p in parts]
    try:
        for p in parts:
            p.concurrent = False
        r = ClipRunner(model, vq, args.batch, n_samples, use_graph=True)
        r(audio)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            r(audio)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps
    finally:
        for p, c in zip(parts, saved):
            p.concurrent = c


def roofline_report(records, precision, ms_per_step, serial_ms=None):
    # An eager bracket [event, kernel, event] also contains the kernel's dispatch gap (~2 us), which a graph replay hides
    # behind the previous kernel: the brackets give the DISTRIBUTION over kernels, their sum is normalised to the measured
    # wall time of the single-stream graph of the same sequence.
    raw_total = sum(r[2] for r in records)
    k = (serial_ms / raw_total) if (serial_ms and raw_total > 0) else 1.0
    records = [(tag, sc, ms * k, flops, byts) for tag, sc, ms, flops, byts in records]
    fam = {}
    for tag, sc, ms, flops, byts in records:
        f = fam.setdefault(tag, [0, 0.0, 0.0, 0.0])
        f[0] += 1
        f[1] += ms
        f[2] += flops
        f[3] += byts
    total_ms = sum(v[1] for v in fam.values())
    name, (cnt, ms, flops, byts) = max(fam.items(), key=lambda kv: kv[1][1])
    mfma_peak = F32_MFMA_PEAK_TFLOPS if precision == "fp32" else F16_MFMA_PEAK_TFLOPS
    if flops > 0 and name in ("emage_gemm", "emage_attention", "emage_conv_slab"):
        ach = flops / (ms * 1e-3) / 1e12
        roof = {"bound": "mfma", "achieved": ach, "peak": mfma_peak, "unit": "TFLOP/s", "frac": ach / mfma_peak}
    else:
        ach = byts / (ms * 1e-3) / 1e9
        roof = {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS}
    traffic, traffic_source = None, None
    tfile = os.path.join(ROOT, "profiles", "hbm_traffic.json")
    if os.path.exists(tfile):
        with open(tfile) as f:
            tj = json.load(f)
        traffic = tj.get(f"{name}:{precision}")
        roof["traffic_collected_on"] = {"commit": tj.get("_commit"), "kernel_sources_sha": tj.get("_kernel_sources_sha"), "gpu_call": tj.get("_gpu_call")}
        roof["kernel_sources_sha_now"] = kernel_sources_sha()
        roof["traffic_is_stale"] = (tj.get("_kernel_sources_sha") != roof["kernel_sources_sha_now"])
        if roof["traffic_is_stale"]:
            log("WARNING: profiles/hbm_traffic.json was collected on other kernel sources than this tree's (roofline.traffic_is_stale)")
        if traffic is not None:
            traffic_source = ("STATIC — not measured in this run: bytes per launch read from profiles/hbm_traffic.json ("
                              + str(tj.get("_source", "rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE passes over bench.py, (2 x FETCH_SIZE + WRITE_SIZE) x 1024 per the microarch guide"))
                              + "); PMC counters cannot be collected from inside the timed process")
    roof.update({
        "traffic": traffic, "traffic_source": traffic_source, "kernel": name, "launches_per_step": cnt, "avg_launch_us": 1e3 * ms / cnt,
        "algorithmic_gflop_per_launch": flops / cnt / 1e9, "algorithmic_mb_per_launch": byts / cnt / 1e6,
        "traffic_over_algorithmic": (traffic / (byts / cnt)) if (traffic and byts > 0) else None,
        "note": "algorithmic flops (2*M*N*K, unpadded K) / serialized kernel time; in f16x3 every product issues 3 MFMAs, so the "
                "MFMA pipes are busy for about 3x this fraction",
        "how": "the timed launch sequence captured as a SINGLE-stream hipGraph and timed (serialized_kernel_ms = its wall time per step = "
               "sum of kernel device times); its split over kernels from one extra eager pass with a HIP-event pair per kernel (device "
               "backlogged so the host runs ahead), normalised to that wall time (the eager brackets also contain each kernel's ~2 us "
               "dispatch gap: event_bracket_sum_ms).  The timed region replays the same sequence with independent chains on parallel "
               "graph branches, hence ms_per_step < serialized_kernel_ms",
        "serialized_kernel_ms": total_ms, "event_bracket_sum_ms": raw_total, "timed_ms_per_step": ms_per_step,
        "share_of_kernel_time": ms / total_ms if total_ms else None,
        "kernel_time_ms_by_family": {k: round(v[1], 3) for k, v in sorted(fam.items(), key=lambda kv: -kv[1][1])},
        "launches_by_family": {k: v[0] for k, v in fam.items()},
    })
    # north_star: MFMA utilisation of the transformer blocks, achieved GB/s of the VQ arg-min
    tb = [r for r in records if r[1] == "transformer_blocks"]
    tb_ms, tb_flops = sum(r[2] for r in tb), sum(r[3] for r in tb)
    if tb_ms > 0:
        roof["transformer_blocks"] = {"launches": len(tb), "ms": tb_ms, "algorithmic_gflop": tb_flops / 1e9,
                                      "achieved_tflops": tb_flops / (tb_ms * 1e-3) / 1e12,
                                      "frac_of_mfma_peak": tb_flops / (tb_ms * 1e-3) / 1e12 / mfma_peak,
                                      "target": 0.40,
                                      "scope": "16 layers x 2 windows: their GEMMs (incl. memory K/V projections), attention, LayerNorm"}
    vq = fam.get("emage_vq_argmin")
    if vq:
        roof["vq_argmin"] = {"in_step": {"launches": vq[0], "avg_us": 1e3 * vq[1] / vq[0], "achieved_gbs": vq[3] / (vq[1] * 1e-3) / 1e9,
                                          "bytes_per_launch": vq[3] / vq[0]}}
    return roof


def vq_argmin_large(device, n=1 << 20, iters=5):
    """the arg-min's HBM figure is only meaningful at N >= 1 M vectors (at N = 4096 it is launch-bound)."""
    from pantomatrix_amd import ops
    g = torch.Generator().manual_seed(3)
    z = torch.randn(n, 256, generator=g).to(device)
    cb = torch.randn(256, 256, generator=g).to(device)
    idx = torch.empty(n, dtype=torch.int64, device=device)
    ops.vq_argmin(z, cb, out=idx)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        ops.vq_argmin(z, cb, out=idx)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    byts = n * 256 * 4 + 256 * 256 * 4 + n * 8
    return {"n": n, "ms": ms, "achieved_gbs": byts / (ms * 1e-3) / 1e9, "frac_of_hbm_peak": byts / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
            "fp32_mfma_tflops": 2.0 * n * 256 * 256 / (ms * 1e-3) / 1e12}


def code_agreement(model, vq, audio, batch):
    """VQ code indices of THIS run against the REFERENCE's run of the same 64-clip batch (tests/golden/infer_128f_b64.npz, generated from the real
    reference by tests/golden/make_golden.py; rank 0's synthetic batch is that batch): the fraction of equal codes per part and of frames whose
    three body codes all agree.  1.0 everywhere = north_star's "bit-exact on VQ code indices"."""
    from tools import workloads as common
    path = os.path.join(ROOT, "tests", "golden", "infer_128f_b64.npz")
    if batch != 64 or not os.path.exists(path):
        return {"skipped": "needs the 64-clip BASELINE batch and tests/golden/infer_128f_b64.npz"}
    g = np.load(path)
    _res, lat = common.product_infer_clip(model, vq, audio)
    sel = model._select_codes(lat)
    out, frames_ok = {}, None
    for part in ("upper", "hands", "lower"):
        eq = sel[f"{part}_index"].cpu().numpy() == g[f"index_{part}"].astype(np.int64)
        out[part] = float(eq.mean())
        frames_ok = eq if frames_ok is None else (frames_ok & eq)
    from pantomatrix_amd.modeling_emage_audio import _Ctx
    face = vq.vq_model_face._nearest(_Ctx(vq.vq_model_face._engine()), lat["rec_face"].reshape(-1, 256).contiguous())
    out["face"] = float((face.view(batch, -1).cpu().numpy() == g["index_face"].astype(np.int64)).mean())
    out["frames_with_all_body_codes_equal"] = float(frames_ok.mean())
    out["codes_compared"] = int(4 * frames_ok.size)
    out["against"] = "tests/golden/infer_128f_b64.npz (the real reference's fp32 CPU run of the same batch)"
    return out


def kernel_sources_sha():
    """sha256 (16 hex digits) over the kernel sources the traffic figures depend on: pantomatrix_amd/csrc/*.{hip,h} in name order."""
    import glob
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "pantomatrix_amd", "csrc")
    for f in sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h"))):
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def cpu_baseline(frames, seconds_budget=15.0):
    """The CPU oracle (a port of the reference path, oracle/emage_oracle.py) on a bounded sample of the same
    workload: `bs` 128-frame clips per call, repeated until ~seconds_budget of CPU work."""
    from tools import workloads as common
    from oracle import emage_oracle as orc
    from pantomatrix_amd import synthetic
    # use the cores this container may actually run on (affinity AND cgroup CPU quota): forcing os.cpu_count()
    # threads on a quota-limited box measures the scheduler, not the code
    torch.set_num_threads(usable_cores())
    omodel, ovq = common.oracle_models()
    t0 = time.time()
    orc.infer_clip(omodel, ovq, synthetic.synthetic_audio(1, synthetic.samples_for_frames(frames)))   # warm-up
    t_one = time.time() - t0
    log(f"cpu_baseline: warm-up clip took {t_one:.2f}s with {torch.get_num_threads()} threads")
    bs = 8 if t_one < 1.0 else (2 if t_one < 4.0 else 1)
    audio = synthetic.synthetic_audio(bs, synthetic.samples_for_frames(frames))
    times, out_frames, t_start = [], 0, time.time()
    while True:
        t0 = time.time()
        poses, _, _ = orc.infer_clip(omodel, ovq, audio)
        times.append(time.time() - t0)
        out_frames = poses.shape[0] * poses.shape[1]
        if time.time() - t_start > seconds_budget or len(times) >= 200:
            break
    med = float(np.median(times))
    b64 = None
    if t_one < 2.0:                       # the headline batch itself, ONCE (the same inputs; the survey measured ~7 s on 8 cores)
        a64 = synthetic.synthetic_audio(64, synthetic.samples_for_frames(frames))
        t0 = time.time()
        p64, _, _ = orc.infer_clip(omodel, ovq, a64)
        dt = time.time() - t0
        b64 = {"value": p64.shape[0] * p64.shape[1] / dt, "unit": "motion-frames/s", "seconds": dt, "sample": f"64 clips x {frames} frames, one call: the batch `value` is quoted on"}
        log(f"cpu_baseline: the 64-clip batch took {dt:.1f}s")
    return {"value": out_frames / med, "unit": "motion-frames/s", "cores": torch.get_num_threads(), "kind": "port", "b64": b64,
            "sample": f"{bs} clips x {frames} frames per call (the survey measured B = 64 slower per frame than B = 8 on CPU), "
                      f"median of {len(times)} calls ({sum(times):.1f} s CPU), fp32 torch CPU oracle = a port of the reference "
                      f"(the reference itself cannot travel to this box)"}


# ----------------------------------------------------------------------------------------------------------------------
# BASELINE configs[3] / [4] (DisCo, CaMN inference) and configs[2] (one EMAGE training step), timed beside the headline metric
# ----------------------------------------------------------------------------------------------------------------------
def bench_lstm_models(dev, steps=3, cpu=True):
    """DisCo at batch 128 x 8.5 s clips and CaMN at batch 256 x 28 s clips (BASELINE configs[3], [4]): one step = one hipGraph replay of
    the whole forward (runtime.LstmClipRunner) + D2H of the motion.  `roofline` is the dominant kernel, the persistent recurrence
    `emage_lstm_layer` (one launch per LSTM layer), timed live with HIP events on a bare launch of the model's size: its algorithmic
    flops (2 directions x B x T x 4H x H x 2) against the dense fp16 MFMA peak — every time step ends in a hand-over of h_t between the
    blocks of a group, which is what bounds it (us_per_time_step)."""
    from pantomatrix_amd import ops, synthetic
    from pantomatrix_amd._lib import F16X3
    from pantomatrix_amd.runtime import LstmClipRunner
    from tools.workloads import lstm_product as product, lstm_weights as weights, lstm_oracle as run_oracle
    out = {}
    for kind, batch, seconds in (("disco", 128, 8.5), ("camn", 256, 28.0)):
        n = int(seconds * 16000)
        model = product(kind, "f16x3", dev)
        audio = synthetic.synthetic_audio(batch, n, seed=5).to(dev)
        runner = LstmClipRunner(model, batch, n)
        runner(audio)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            motion, _aa = runner(audio)
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0) / steps
        tt, frames = int(motion.shape[1]), int(motion.shape[0] * motion.shape[1])
        line = {"workload": f"{kind} inference f16x3, batch={batch} x {seconds} s synthetic clips (BASELINE configs[{3 if kind == 'disco' else 4}])",
                "ms_per_step": ms, "value": frames / (ms * 1e-3), "unit": "motion-frames/s (15 fps)", "frames_per_clip": tt, "steps": steps,
                "dtype": "f16x3", "launch": "hipGraph replay"}
        hid = 512
        g = torch.Generator().manual_seed(1)
        wp, ws = [], []
        for _ in range(2):
            p_, s_ = ops.split_f16_weights(torch.randn(4 * hid, hid, generator=g) / hid ** 0.5)
            wp.append(p_.to(dev))
            ws.append(s_)
        gx = torch.randn(batch, tt, 8 * hid, generator=g).to(dev)
        hseq = torch.empty(batch, tt, 2 * hid, device=dev)
        sync = ops.lstm_layer_sync(batch, hid, dev)
        ops.lstm_layer(F16X3, gx, wp, ws, hseq, sync)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(3):
            ops.lstm_layer(F16X3, gx, wp, ws, hseq, sync)
        e1.record()
        torch.cuda.synchronize()
        ops.lstm_layer_check(sync)
        layer_ms = e0.elapsed_time(e1) / 3
        flops = 2.0 * batch * tt * 4 * hid * hid * 2
        n_layers = (1 if kind == "disco" else 2) * 4
        line["roofline"] = {"bound": "mfma", "kernel": "emage_lstm_layer", "achieved": flops / (layer_ms * 1e-3) / 1e12, "peak": 2500.0, "unit": "TFLOP/s",
                            "frac": flops / (layer_ms * 1e-3) / 1e12 / 2500.0, "traffic": None, "launch_ms": layer_ms, "launches_per_step": n_layers,
                            "share_of_step": n_layers * layer_ms / ms, "us_per_time_step": 1e3 * layer_ms / tt,
                            "note": "algorithmic flops of one bidirectional layer (2 x B x T x 4H x H x 2) / its launch time; 3 MFMAs per product; a time "
                                    "step is bound by the h_t hand-over between the blocks of a group, not by MFMA issue"}
        del gx, hseq
        if cpu:
            torch.set_num_threads(usable_cores())
            sd = weights(kind)
            a2 = audio[:2].cpu()
            spk = torch.zeros(2, 1, dtype=torch.long)
            run_oracle(kind, sd, a2[:, :n // 4], spk, None)
            t0 = time.time()
            ref = run_oracle(kind, sd, a2, spk, None)
            dt = time.time() - t0
            line["cpu_baseline"] = {"value": 2 * ref["motion"].shape[1] / dt, "unit": "motion-frames/s (15 fps)", "kind": "port", "cores": torch.get_num_threads(),
                                    "sample": f"2 clips x {seconds} s, one call ({dt:.1f} s CPU), fp32 torch CPU oracle (oracle/lstm_models_oracle.py)"}
            line["max_err_vs_oracle_clips_0_1"] = float((torch.from_numpy(motion[:2]) - ref["motion"].reshape(2, -1, 258)).abs().max())
        out[kind] = line
        del runner, model, audio
        torch.cuda.empty_cache()
    return out


def bench_exchange_single_rank(dev, data, random_mask, steps=3):
    """`Trainer(sync_bn=True, exchange=True)` in a WORLD_SIZE = 1 `nccl` (= RCCL) process group on this GPU: collectives per step, bytes per
    bucket message, the eager step and the step captured WITH its collectives (VERDICT round 4, next #3c).  No multi-GPU node is needed for
    the exchange to run on hardware; the xGMI part of a real ring (2 x 7/8 x 508 MB per GPU and step at ~150 GB/s per link pair: ~6 ms,
    three of four buckets overlapped with the third backward) is arithmetic, stated in DESIGN.md section 8."""
    import torch.distributed as tdist
    from tools import workloads as common
    from pantomatrix_amd import dist as pdist
    from pantomatrix_amd import training
    created = False
    if not tdist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ["MASTER_PORT"] = str(free_port())
        tdist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
        created = True
    try:
        out = {"backend": str(tdist.get_backend()), "world": tdist.get_world_size()}
        model, vq = common.product_models(precision="f16x3", device=dev)
        trainer = training.Trainer(model, vq, seed=1, sync_bn=True, exchange=True)
        with pdist.CollectiveCounter() as cc:
            trainer.step(data, random_mask=random_mask)
        out["collectives_per_step"] = {k: v for k, v in cc.counts.items() if k != "bucket_bytes"}
        out["bucket_bytes"] = trainer.buckets.nbytes()
        out["bytes_all_reduced_per_step"] = cc.counts["bucket_bytes"]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(2):
            trainer.step(data, random_mask=random_mask)
        torch.cuda.synchronize()
        out["eager_ms_per_step"] = 1e3 * (time.perf_counter() - t0) / 2
        trainer.capture(data, random_mask)
        trainer.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            losses = trainer.replay()
        torch.cuda.synchronize()
        out["captured_ms_per_step"] = 1e3 * (time.perf_counter() - t0) / steps
        out["loss_all_after_replays"] = losses["all"]
        out["note"] = ("single-rank RCCL: every collective of the step runs on the device (the all-reduces are the identity); captured = the collectives "
                       "are nodes of the step's hipGraph — what each rank of a multi-GPU run replays (Trainer.capture no longer refuses world > 1 / sync_bn)")
        del trainer, model, vq
        return out
    finally:
        if created:
            tdist.destroy_process_group()


def bench_train_step(dev, steps=3, cpu=True, batch=56, eager=True, accumulate_dw=None, defer_finalize=None, exchange=True, h2_forward=None, direct_conv_dx=None, fuse_grad_adds=None):
    """One EMAGE optimisation step at BASELINE configs[2]'s per-GPU batch (56 clips x 64 frames): targets through the frozen VQ-VAEs, three
    train-mode forwards (batch-statistics BatchNorm, dropout masks drawn on the device), six losses, three backward passes, multi-tensor
    Adam, BatchNorm buffers — `training.Trainer.capture` / `replay`: the whole step is ONE hipGraph.  `roofline`: the step's algorithmic
    flops (9 x 20.5 GFLOP per clip-window + 1.16 GFLOP of VQ encoding) against the dense fp16 MFMA peak (every contraction, forward
    and backward, is split-fp16 MFMA: the backward on EMAGE_H2 operands with power-of-two gradient scaling)."""
    from tools import workloads as common
    from pantomatrix_amd import training
    model, vq = common.product_models(precision="f16x3", device=dev)
    t = 64
    data = {k: v.to(dev) for k, v in common.train_batch(bs=batch, t=t).items()}
    random_mask = (torch.rand(batch, t, 337, generator=torch.Generator().manual_seed(6)) < 0.5).float().to(dev)
    torch.cuda.reset_peak_memory_stats()
    trainer = training.Trainer(model, vq, seed=1)
    if accumulate_dw is not None:                 # tools/bench_train_step.py A/B
        trainer.fwd.accumulate_dw = bool(accumulate_dw)
    if defer_finalize is not None:
        trainer.fwd.defer_finalize = bool(defer_finalize)
    if h2_forward is not None:
        trainer.fwd.h2_forward = bool(h2_forward)
    if direct_conv_dx is not None:
        trainer.fwd.direct_conv_dx = bool(direct_conv_dx)
    if fuse_grad_adds is not None:
        trainer.fwd.fuse_grad_adds = bool(fuse_grad_adds)
    trainer.capture(data, random_mask)
    losses = trainer.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        losses = trainer.replay()
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    assert all(np.isfinite(v) for v in losses.values())
    flops = batch * (9 * 20.5e9 + 1.16e9)
    line = {"workload": f"EMAGE training step f16x3, {batch} x {t}-frame synthetic clips per GPU (BASELINE configs[2] per-GPU batch), one hipGraph replay per step",
            "ms_per_step": ms, "value": batch / (ms * 1e-3), "unit": "clip-windows/s", "steps": steps, "dtype": "f16x3",
            "peak_memory_gb": torch.cuda.max_memory_allocated() / 2 ** 30, "loss_all_after_replays": losses["all"], "replays": steps + 1,
            "skipped_steps": trainer.skipped_steps, "operand_rescales": trainer.rescaled,
            "roofline": {"bound": "mfma", "kernel": "emage_gemm (split-fp16 MFMA, 3 per product: every contraction of the forward and the backward)",
                         "achieved": flops / (ms * 1e-3) / 1e12, "peak": 2500.0, "unit": "TFLOP/s", "frac": flops / (ms * 1e-3) / 1e12 / 2500.0, "traffic": None,
                         "note": "whole-step algorithmic flops / step time (an upper bound on the GEMM family's share) against the dense fp16 MFMA peak"}}
    del trainer
    torch.cuda.empty_cache()
    # the EAGER step — the same launches issued from Python (until round 4 the only form of a multi-process run; round 5 captures the collectives
    # too: `exchange` below) — same model, same inputs, same process: the ratio is this host's (`host` in the line)
    try:
        if not eager:
            raise RuntimeError("not timed in this run")
        eager = training.Trainer(model, vq, seed=1)
        eager.step(data, random_mask=random_mask)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(2):
            eager.step(data, random_mask=random_mask)
        torch.cuda.synchronize()
        ems = 1e3 * (time.perf_counter() - t0) / 2
        line["eager"] = {"ms_per_step": ems, "ratio_to_captured": ems / ms,
                         "note": "Trainer.step: the same launches issued from Python, one host read of losses + health word per step; measured in the SAME process "
                                 "as the captured figure — the ratio depends on the host CPU (`host`), not on the GPU"}
        del eager
    except Exception as exc:                      # noqa: BLE001 — an extra never costs the line
        line["eager"] = {"error": f"{type(exc).__name__}: {exc}"}
    del model, vq
    torch.cuda.empty_cache()
    # the exchange of BASELINE configs[2] (train_emage_audio.py:214, 248-251: DDP + SyncBatchNorm) through RCCL on THIS GPU: a process group of
    # one rank — the four bucket all-reduces, the SyncBatchNorm all-gathers / small all-reduces run on the device, eagerly and inside the
    # captured graph (the form every rank of a multi-GPU run replays)
    try:
        if exchange:
            with native_stdout_to_stderr():      # RCCL's version banner goes to stderr, not next to the JSON line
                line["exchange"] = bench_exchange_single_rank(dev, data, random_mask, steps)
    except Exception as exc:                      # noqa: BLE001
        line["exchange"] = {"error": f"{type(exc).__name__}: {exc}"[:400]}
    torch.cuda.empty_cache()
    if cpu:
        torch.set_num_threads(usable_cores())
        t0 = time.time()
        ref = common.oracle_train_step_recorded(seed=1, iteration=0, bs=2, backward=True)
        dt = time.time() - t0
        line["cpu_baseline"] = {"value": 2 / dt, "unit": "clip-windows/s", "kind": "port", "cores": torch.get_num_threads(),
                                "sample": f"one step on 2 clips ({dt:.1f} s CPU), fp32 torch CPU oracle (oracle/emage_train_oracle.py: a restatement of train_val_fn)"}
        # the same step on the device (eager f16x3, the oracle's recorded dropout draws): losses and gradient norms against the oracle's
        model, vq = common.product_models(precision="f16x3", device=dev)
        got = {}
        dl = training.Trainer(model, vq).step({k: v.to(dev) for k, v in ref["batch"].items()}, 0, [[m.to(dev).contiguous() for m in fm] for fm in ref["masks"]],
                                              ref["random_mask"].to(dev), grad_hook=lambda gr: got.update({k: float(v.norm()) for k, v in gr.items()}))
        gmax = max(float(g.abs().max()) for g in ref["grads"].values())
        live = [k for k, g in ref["grads"].items() if float(g.abs().max()) >= 1e-5 * gmax and not k.startswith(("audio_encoder_face.", "audio_encoder_body."))]
        line["max_rel_loss_err_vs_oracle_2_clips"] = max(abs(dl[k] - v) / max(1.0, abs(v)) for k, v in ref["losses"].items())
        line["max_rel_grad_norm_err_vs_oracle_2_clips"] = max(abs(got[k] - float(ref["grads"][k].norm())) / float(ref["grads"][k].norm()) for k in live)
        line["grad_tensors_compared"] = len(live)
        del model, vq
        torch.cuda.empty_cache()
    return line


def bench_train_step_ranks(dev, world, rank, barrier, reduce_max, steps=3, warmup=1, batch=56, t=64, captured=None, models=None, prepare=None):
    """BASELINE configs[2] at N ranks (train_emage_audio.py:214, 248-251, 275-276: DistributedDataParallel + SyncBatchNorm): EVERY rank calls
    this behind an initialised process group.  Two arms on the same model and per-rank data (`batch` clips x `t` frames per rank: weak scaling),
    each timed like the headline figure — barrier, `steps` steps, barrier, max over ranks:

      with_exchange     Trainer(sync_bn=True, exchange=True): the four backward-ordered bucket all-reduces (started mid-backward), SyncBatchNorm's
                        all-gathers / small all-reduces; on the `nccl` (= RCCL) backend the step is ONE hipGraph per rank whose nodes include
                        the collectives (Trainer.capture), on any other backend (gloo: the CPU tests) the eager Trainer.step;
      without_exchange  Trainer(sync_bn=False, exchange=False): the same step with no collective at all (each rank on its own).

    exposed_exchange_ms = with - without: what the collectives cost BEHIND the overlap with the third backward.  `value` = clip-windows/s summed
    over ranks.  `captured` None: by backend; `models` / `prepare`: test hooks (the CPU stand-ins)."""
    import torch.distributed as tdist
    from tools import workloads as common
    from pantomatrix_amd import dist as pdist
    from pantomatrix_amd import training
    backend = str(tdist.get_backend())
    if captured is None:
        captured = backend == "nccl"
    model, vq = models if models is not None else common.product_models(precision="f16x3", device=dev)
    data = {k: v.to(dev) for k, v in common.train_batch(bs=batch, t=t, seed=5 + rank).items()}      # every rank its own clips
    random_mask = (torch.rand(batch, t, 337, generator=torch.Generator().manual_seed(6 + rank)) < 0.5).float().to(dev)
    out = {"workload": f"EMAGE training step f16x3, {batch} x {t}-frame synthetic clips PER RANK on {world} rank(s) (BASELINE configs[2]: DDP + SyncBatchNorm), "
                       + ("one hipGraph replay per step and rank, collectives inside the graph" if captured else "eager Trainer.step"),
           "backend": backend, "world": world, "steps": steps, "dtype": "f16x3", "launch": "hipGraph replay" if captured else "eager"}
    arms = {}
    for arm, kw in (("with_exchange", dict(sync_bn=True, exchange=True)), ("without_exchange", dict(sync_bn=False, exchange=False))):
        trainer = training.Trainer(model, vq, seed=1, **kw)
        if prepare is not None:
            prepare(trainer)
        counts = None
        if captured:
            trainer.capture(data, random_mask)
            step = trainer.replay
        else:
            step = lambda trainer=trainer: trainer.step(data, random_mask=random_mask)
        with pdist.CollectiveCounter() as cc:                 # the first step: eager = the collectives of a step; captured = none (they are graph nodes)
            losses = step()
        counts = {k: v for k, v in cc.counts.items()}
        elapsed, losses = timed_steps(step, steps, max(0, warmup - 1), barrier, reduce_max)      # the counted step above was the first warm-up
        ms = 1e3 * elapsed / steps
        arms[arm] = {"ms_per_step": ms, "value": batch * world / (ms * 1e-3), "unit": "clip-windows/s", "loss_all_rank0": losses["all"],
                     "skipped_steps": trainer.skipped_steps}
        if arm == "with_exchange":
            arms[arm]["bucket_bytes"] = trainer.buckets.nbytes()
            arms[arm]["bytes_all_reduced_per_step_and_rank"] = int(sum(trainer.buckets.nbytes()))
            if not captured:
                arms[arm]["collectives_per_step"] = {k: v for k, v in counts.items() if k != "bucket_bytes"}
            else:
                arms[arm]["collectives_per_step"] = "4 bucket all-reduces + 12 SyncBatchNorm all-gathers + 13 small all-reduces, nodes of the graph (counts pinned by tests/test_rccl_gpu.py)"
        del trainer
        if dev is not None and getattr(dev, "type", "cpu") == "cuda":
            torch.cuda.empty_cache()
    out.update(arms)
    w, wo = arms["with_exchange"]["ms_per_step"], arms["without_exchange"]["ms_per_step"]
    out["ms_per_step"], out["value"], out["unit"] = w, arms["with_exchange"]["value"], "clip-windows/s"
    out["exposed_exchange_ms"] = w - wo
    flops = batch * (9 * 20.5e9 + 1.16e9) * world
    out["roofline"] = {"bound": "mfma", "achieved": flops / (w * 1e-3) / 1e12, "peak": F16_MFMA_PEAK_TFLOPS * world, "unit": "TFLOP/s",
                       "frac": flops / (w * 1e-3) / 1e12 / (F16_MFMA_PEAK_TFLOPS * world), "traffic": None,
                       "note": "whole-job algorithmic flops of the step / step time against world x the dense fp16 MFMA peak"}
    out["xgmi_arithmetic"] = ("ring all-reduce: 2 x (N-1)/N x bytes per GPU and step over ~150 GB/s per xGMI link pair; three of the four buckets "
                              "overlap the third backward (DESIGN.md section 8)")
    return out


CLIP_GFLOP_128 = 44.0          # algorithmic GFLOP of one 128-frame clip end to end (2 x (20.50 + 0.574) + (0.574 + 0.41) x 120 / 64)


def _time_runner(runner, audio, steps, warmup=2):
    """ms per call of `runner(audio)` — the timed region of `value` (graph replay + D2H + one synchronisation), audio resident in HBM."""
    for _ in range(warmup):
        runner(audio)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = runner(audio)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps, out


def bench_config1(precision, dev, args, cpu=True):
    """BASELINE configs[0] / SURVEY 8(d) "config 1" on the DEVICE — the shape test_emage_audio.py:16-56 actually runs: ONE clip.
    (i) B = 1 x 128 frames (2 dependent windows + the final decode); (ii) B = 1 x 28 s (448 000 samples = 840 frames: 14 dependent
    windows of M = 64 rows each).  Graph replay, same timed region as `value`; the CPU oracle at B = 1 beside it."""
    from pantomatrix_amd import synthetic
    from pantomatrix_amd.runtime import ClipRunner
    from tools import workloads as common
    model, vq = common.product_models(precision=precision, device=dev)
    out = {"workload": "EMAGE inference, ONE clip (BASELINE configs[0], test_emage_audio.py:16-56): graph replay, audio resident in HBM, results on the host",
           "dtype": precision}
    for key, n_samples in (("b1_128f", synthetic.samples_for_frames(128)), ("b1_28s", 448000)):
        runner = ClipRunner(model, vq, 1, n_samples, use_graph=not args.no_graph, split_k=args.split_k)
        audio = synthetic.synthetic_audio(1, n_samples, seed=1234).to(dev)
        ms, res = _time_runner(runner, audio, steps=max(5, args.steps))
        frames = int(res[0].shape[1])
        rounds = (n_samples * 30 // 16000 - 4) // 60
        out[key] = {"ms": ms, "frames_out": frames, "frames_per_s": frames / (ms * 1e-3), "windows": rounds + (1 if frames > rounds * 60 else 0),
                    "ms_per_window": ms / max(1, rounds), "samples": n_samples}
        del runner
        torch.cuda.empty_cache()
    out["bound"] = ("latency: a window is ~280 dependent launches of M = 64 rows (one 64-row tile column per contraction: <= 36 of 256 CUs busy); "
                    "ms_per_window / ~280 launches = the per-launch floor of a dependent chain inside a hipGraph")
    if cpu:
        from oracle import emage_oracle as orc
        torch.set_num_threads(usable_cores())
        omodel, ovq = common.oracle_models()
        a1 = synthetic.synthetic_audio(1, synthetic.samples_for_frames(128), seed=1234)
        orc.infer_clip(omodel, ovq, a1)
        ts = []
        for _ in range(3):
            t0 = time.time()
            poses, _, _ = orc.infer_clip(omodel, ovq, a1)
            ts.append(time.time() - t0)
        out["cpu_baseline_b1_128f"] = {"value": poses.shape[1] / float(np.median(ts)), "unit": "motion-frames/s", "cores": torch.get_num_threads(), "kind": "port",
                                       "sample": f"1 clip x 128 frames, median of 3 calls ({sum(ts):.1f} s CPU), fp32 torch CPU oracle"}
    del model, vq
    torch.cuda.empty_cache()
    return out


def bench_batch_sweep(precision, dev, args, batches=(1, 8, 64, 256)):
    """Throughput against the batch: B clips x 128 frames per step, graph replay, the timed region of `value`.  `frac_whole_step` = B x 44.0
    GFLOP (algorithmic) / step time against the dense fp16 MFMA peak — where the launch-bound regime ends and what the chip
    reaches when every contraction has 4x the rows of the BASELINE batch."""
    from pantomatrix_amd import synthetic
    from pantomatrix_amd.runtime import ClipRunner
    from tools import workloads as common
    model, vq = common.product_models(precision=precision, device=dev)
    n_samples = synthetic.samples_for_frames(128)
    out = {"workload": "EMAGE inference, B x 128-frame clips per step (graph replay, audio resident in HBM)", "dtype": precision, "by_batch": {}}
    for b in batches:
        try:
            runner = ClipRunner(model, vq, b, n_samples, use_graph=not args.no_graph, split_k=args.split_k)
            audio = synthetic.synthetic_audio(b, n_samples, seed=1234).to(dev)
            ms, res = _time_runner(runner, audio, steps=max(3, args.steps // 2))
            frames = int(res[0].shape[0] * res[0].shape[1])
            tf = b * CLIP_GFLOP_128 * 1e9 / (ms * 1e-3) / 1e12
            out["by_batch"][str(b)] = {"ms_per_step": ms, "frames_per_s": frames / (ms * 1e-3), "achieved_tflops_whole_step": tf,
                                       "frac_whole_step": tf / F16_MFMA_PEAK_TFLOPS}
            del runner, audio
        except Exception as e:  # noqa: BLE001
            out["by_batch"][str(b)] = {"error": f"{type(e).__name__}: {e}"[:300]}
        torch.cuda.empty_cache()
    ok = {int(k): v for k, v in out["by_batch"].items() if "frames_per_s" in v}
    if len(ok) >= 2:
        ks = sorted(ok)
        out["saturation"] = {f"{a}->{b}": ok[b]["frames_per_s"] / ok[a]["frames_per_s"] for a, b in zip(ks, ks[1:])}
    del model, vq
    torch.cuda.empty_cache()
    return out


def host_info():
    import platform
    model = ""
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                model = ln.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return {"node": platform.node(), "cpu": model, "usable_cores": usable_cores(), "os_cpu_count": os.cpu_count()}


def build(precision, device, args):
    from tools import workloads as common
    from pantomatrix_amd import synthetic
    from pantomatrix_amd.runtime import ClipRunner
    model, vq = common.product_models(precision=precision, device=device)
    model.hoist_audio = not args.no_hoist
    model.slab_convs = not args.no_slab_convs
    for part in (model, vq.vq_model_face, vq.vq_model_upper, vq.vq_model_hands, vq.vq_model_lower, vq.global_motion):
        part.split_acts = not args.no_split_acts
    model.h2_residual = not args.f32_residual
    model.fold_layernorm = not args.no_fold_ln
    for part in (model, vq.vq_model_face, vq.vq_model_upper, vq.vq_model_hands, vq.vq_model_lower, vq.global_motion):
        part.concurrent = not args.no_concurrent
        part.group_gemms = not args.no_group_gemms
    if args.group_face_body is not None:
        model.group_face_body = bool(args.group_face_body)
    n_samples = synthetic.samples_for_frames(args.frames)
    runner = ClipRunner(model, vq, args.batch, n_samples, use_graph=not args.no_graph, main_priority=args.main_priority)
    return model, vq, runner, n_samples


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true", help="also run every measurement beyond the headline line (PCIe-inclusive rate, roofline, "
                                                        "code agreement, other precisions, CPU baselines, config 1, batch sweep, DisCo / CaMN, "
                                                        "training step); the --no-* switches below trim it")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the last timed step's results (rank 0) as DIR/<name>.npy, float32")
    ap.add_argument("--batch", type=int, default=64, help="clips per GPU per step (BASELINE config 2: 64)")
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--precision", default="f16x3", choices=["f16x3", "bf16", "fp32"],
                    help="f16x3 (default): fp32 storage, split-f16 MFMA — the parity-green fast mode; bf16: bf16 operands "
                         "(not index-exact); fp32: exact-fp32 MFMA")
    ap.add_argument("--also", default="bf16", help="comma list of further precisions timed beside the reported one ('' = none)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-other-configs", action="store_true", help="skip the DisCo / CaMN inference and the EMAGE training-step lines (BASELINE configs[2..4])")
    ap.add_argument("--no-hoist", action="store_true", help="A/B: compute waveform features inside every window")
    ap.add_argument("--no-slab-convs", action="store_true", help="A/B: WavEncoder through emage_wav_conv_in + emage_gemm only (same bits)")
    ap.add_argument("--main-priority", action="store_true", help="experiment: capture the clip graph on a high-priority stream")
    ap.add_argument("--gemm-variant", type=int, default=-1, help="experiments: emage_set_tuning key 2 (tile-heuristic variant)")
    ap.add_argument("--gemm-dbg", type=int, default=0, help="experiments: emage_set_tuning key 1 mask (8: sc1 result stores, 16: nt)")
    ap.add_argument("--no-split-acts", action="store_true", help="A/B: float32 activations split inside every GEMM (EMAGE_F16X3) instead of pre-split EMAGE_H2 storage")
    ap.add_argument("--pipeline", type=int, default=1, help="also time the step with this many batches in flight (runtime.ClipPipeline)")
    ap.add_argument("--f32-residual", action="store_true", help="A/B: float32 residual twins beside the EMAGE_H2 images (round 3's default) instead of residuals read from the images")
    ap.add_argument("--group-face-body", type=int, default=None, help="A/B (default: the class default): 1 = the face decoder layers walk in lock step with the first cross-attention layers (shared launches, one lane); 0 = two stream lanes")
    ap.add_argument("--no-group-gemms", action="store_true", help="A/B: one stream lane per part-wise chain and one launch per contraction instead of lock-step chains with grouped launches")
    ap.add_argument("--attn-variant", type=int, default=0, help="experiments: emage_set_tuning key 6 (1 = split-f16 attention without the LDS-staged K / V^T)")
    ap.add_argument("--h2-variant", type=int, default=0, help="experiments: emage_set_tuning key 5 (EMAGE_H2 tile-heuristic variant)")
    ap.add_argument("--tools-lib", action="store_true", help="experiments: run on libemage_hip_tools.so even with every tuning key at its default (the fair A arm of a tools-library A/B)")
    ap.add_argument("--h2-pp", type=int, default=0, help="experiments: emage_set_tuning key 8 (antiphase tile configuration, gemm_h2_pp.hip, for the 768-wide launches; tools library)")
    ap.add_argument("--split-k", action="store_true", help="A/B (config1 / small batches): in-launch split-K for the few-row contractions (measured slower: off by default)")
    ap.add_argument("--no-fold-ln", action="store_true", help="A/B: every LayerNorm is a launch (round 5's form) instead of folded into the contractions around it")
    ap.add_argument("--no-concurrent", action="store_true", help="A/B / profiling: single stream, no fork/join lanes")
    ap.add_argument("--no-graph", action="store_true", help="launch eagerly instead of replaying the captured hipGraph")
    ap.add_argument("--train", action="store_true", help="run the N-rank training-step leg also at N = 1 (needs a launcher: a process group of one rank on RCCL) - "
                                                         "what every rank of a multi-GPU run does, on the one GPU of a box")
    ap.add_argument("--train-timeout", type=float, default=480.0, help="watchdog of the N-rank training-step leg (seconds)")
    ap.add_argument("--train-batch", type=int, default=56, help="clips per GPU of the training-step leg at N > 1 ranks (BASELINE configs[2]: 56)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # no launcher: become one — one process per GPU, the driver's own torchrun recipe
        if torch.cuda.is_available() and torch.cuda.device_count() < args.gpus:
            raise SystemExit(f"--gpus {args.gpus} but only {torch.cuda.device_count()} GPU(s) visible")
        cmd = spawn_command(sys.argv[1:], args.gpus, free_port())
        log("no launcher in the environment: re-executing as " + " ".join(cmd[1:8]) + " ...")
        raise SystemExit(subprocess.call(cmd))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (torch.cuda.is_available() is False); there is no CPU path")
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} does not match WORLD_SIZE {world}: launch with --nproc-per-node {args.gpus}")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    from pantomatrix_amd import dist as pdist
    from pantomatrix_amd import synthetic

    if args.gemm_dbg or args.gemm_variant >= 0 or args.h2_variant or args.attn_variant or args.h2_pp or args.tools_lib:
        from pantomatrix_amd import _lib
        _lib.use_tools(True)         # experiments only: the tuning hooks live in the tools build of the library
        _lib.load().emage_set_tuning(1, args.gemm_dbg)
        _lib.load().emage_set_tuning(5, args.h2_variant)
        _lib.load().emage_set_tuning(6, args.attn_variant)
        _lib.load().emage_set_tuning(8, args.h2_pp)
        if args.gemm_variant >= 0:
            _lib.load().emage_set_tuning(2, args.gemm_variant)
    log(f"rank {rank}/{world}: building the {args.precision} models on {dev} and capturing the clip graph")
    model, vq, runner, n_samples = build(args.precision, dev, args)
    # clip i of the global batch lives on rank i % world; every rank gets `batch` clips (weak scaling)
    audio_host = synthetic.synthetic_audio(args.batch, n_samples, seed=1234 + rank).pin_memory()
    audio = audio_host.to(dev)
    # the process group (RCCL; barriers and the max-over-ranks of the timing only) is joined AFTER the graph capture, so
    # no communicator thread is alive while the stream capture is open; None without a launcher
    with native_stdout_to_stderr():          # the backend's banner must not reach stdout (one JSON line there)
        if pdist.init("nccl", dev) is not None:
            pdist.barrier()                  # the communicator (and its banner) is created by the first collective
            torch.cuda.synchronize()

    def barrier():
        pdist.barrier()
        torch.cuda.synchronize()

    reduce_max = lambda v: pdist.max_over_ranks(v, dev)
    log(f"warm-up x{args.warmup}, then {args.steps} timed steps")
    elapsed, out = timed_steps(lambda: runner(audio), args.steps, args.warmup, barrier, reduce_max)
    poses = out[0]
    frames_per_step = poses.shape[0] * poses.shape[1]
    assert np.isfinite(poses).all()
    log(f"timed: {1e3 * elapsed / args.steps:.2f} ms/step")
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, out)
    result = result_line(args.precision, elapsed, args.steps, args.warmup, world, frames_per_step, args.batch, args.frames,
                         "eager" if args.no_graph else "hipGraph replay")

    if args.full:
        # the same step with the audio batch crossing PCIe inside the timed region (pinned host -> HBM), SURVEY §8(d)
        el_pcie, _ = timed_steps(lambda: runner(audio_host), args.steps, 1, barrier, reduce_max)
        result["pcie_inclusive"] = {"value": frames_per_step * world * args.steps / el_pcie, "ms_per_step": 1e3 * el_pcie / args.steps,
                                    "h2d_bytes_per_step": audio_host.numel() * 4,
                                    "note": "SURVEY 8(d)'s definition of the metric (H2D of the audio inside the timed step: pinned host -> HBM in every step, "
                                            "D2H of the three result arrays in both figures).  `value` above is the HBM-resident rate because the document that "
                                            "fixes the bench contract says so — the round's task statement, section (4) Measurement: '`value` is whole-job throughput "
                                            "with inputs already resident in HBM when the timed region starts (if the boundary hands over host buffers, note the "
                                            "PCIe-inclusive rate in DESIGN.md - it is never `value`)' (quoted in DESIGN.md section 6); the figure that conforms to "
                                            "SURVEY 8(d) is THIS object"}

    if args.pipeline > 1:
        from pantomatrix_amd.runtime import ClipPipeline
        pipe = ClipPipeline(model, vq, args.batch, n_samples, depth=args.pipeline, use_graph=not args.no_graph)
        el_p, out_p = timed_pipeline(pipe, audio, args.steps, args.warmup, barrier, reduce_max)
        assert np.array_equal(out_p[0], poses), "pipelined batches must reproduce the one-at-a-time result bit for bit"
        result["pipelined"] = {"depth": args.pipeline, "value": frames_per_step * world * args.steps / el_p, "ms_per_step": 1e3 * el_p / args.steps}
        del pipe

    hard_exit = False

    def guarded(key, fn):
        """The headline measurement above is done: a failure in one of the additional objects is reported in its place, not raised."""
        try:
            result[key] = fn()
        except Exception as e:  # noqa: BLE001
            log(f"{key} failed: {type(e).__name__}: {e}")
            result[key] = {"error": f"{type(e).__name__}: {e}"[:500]}
            torch.cuda.empty_cache()

    if args.full and rank == 0 and not args.no_roofline:
        def roofline():
            records, _marker_ms = profile_kernels(runner, model, vq)
            serial_ms = None if args.no_graph else serialized_graph_ms(model, vq, args, n_samples, audio, args.steps)
            rep = roofline_report(records, args.precision, result["ms_per_step"], serial_ms)
            if world == 1:
                rep.setdefault("vq_argmin", {})["n_1m"] = vq_argmin_large(dev)
            return rep
        guarded("roofline", roofline)
    if args.full and rank == 0 and world == 1 and not args.no_roofline:
        guarded("code_agreement", lambda: code_agreement(model, vq, audio, args.batch))
    if args.full and world == 1 and args.also:
        del runner, model, vq
        torch.cuda.empty_cache()

        def other_precisions():
            others = {}
            for p in [x for x in args.also.split(",") if x and x != args.precision]:
                m2, v2, r2, _ = build(p, dev, args)
                el2, _ = timed_steps(lambda: r2(audio), args.steps, args.warmup, barrier, reduce_max)
                others[p] = {"value": frames_per_step * args.steps / el2, "ms_per_step": 1e3 * el2 / args.steps, "precision": PRECISION_NOTE[p]}
                if not args.no_roofline:
                    # the same measurement as the headline `roofline`, for THIS precision (north_star quotes its 0.40 against bf16 MFMA)
                    try:
                        recs, _mk = profile_kernels(r2, m2, v2)
                        ser = None if args.no_graph else serialized_graph_ms(m2, v2, args, n_samples, audio, args.steps)
                        rep = roofline_report(recs, p, others[p]["ms_per_step"], ser)
                        others[p]["roofline"] = {k: rep.get(k) for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "launches_per_step", "avg_launch_us",
                                                                          "algorithmic_gflop_per_launch", "serialized_kernel_ms", "kernel_time_ms_by_family", "transformer_blocks")}
                    except Exception as e:  # noqa: BLE001
                        others[p]["roofline"] = {"error": f"{type(e).__name__}: {e}"[:300]}
                try:
                    others[p]["code_agreement"] = code_agreement(m2, v2, audio, args.batch)
                except Exception as e:  # noqa: BLE001
                    others[p]["code_agreement"] = {"error": f"{type(e).__name__}: {e}"[:300]}
                del m2, v2, r2
                torch.cuda.empty_cache()
            return others
        guarded("other_precisions", other_precisions)
    if (args.full and world > 1 and not args.no_other_configs) or (args.train and pdist.is_initialized()):
        # BASELINE configs[2] at N ranks: EVERY rank runs the captured 56-clip step with its RCCL collectives (and the same step without them)
        log(f"rank {rank}/{world}: the training step at {world} ranks (DDP bucket all-reduces + SyncBatchNorm inside the captured graph)")
        # Under a WATCHDOG: the leg holds collectives (eager warm-up steps, captured graphs); a rank that fails alone would leave the others in
        # theirs for the backend's timeout and cost the driver the HEADLINE line, which is already measured at this point.  The leg runs in a
        # worker thread; when it has not come back after --train-timeout seconds the line is printed with the error in its place and the
        # process leaves through os._exit (a hung collective cannot be cancelled, `finalize` would wait for it).
        import threading
        box = {}

        def train_leg():
            try:
                torch.cuda.set_device(local_rank)
                box["out"] = bench_train_step_ranks(dev, world, rank, barrier, reduce_max, steps=max(3, min(10, args.steps // 2)), batch=args.train_batch)
            except Exception as e:  # noqa: BLE001
                box["err"] = f"{type(e).__name__}: {e}"[:500]

        th = threading.Thread(target=train_leg, daemon=True)
        th.start()
        th.join(timeout=args.train_timeout)
        if th.is_alive():
            log(f"rank {rank}: the training-step leg did not finish within {args.train_timeout} s: reported as an error; leaving through os._exit after the line")
            result["train_step"] = {"error": f"timeout: the N-rank training-step leg did not finish within {args.train_timeout} s on rank {rank}"}
            hard_exit = True
        elif "err" in box:
            log(f"train_step failed: {box['err']}")
            result["train_step"] = {"error": box["err"]}
            hard_exit = world > 1             # the other ranks may be inside a collective this rank will never join
        else:
            result["train_step"] = box["out"]
    if rank == 0:
        result["host"] = host_info()
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        guarded("cpu_baseline", lambda: cpu_baseline(args.frames))
    if args.full and rank == 0 and world == 1 and not args.no_other_configs:
        # BASELINE configs[0] on the device (one clip: 128 frames and 28 s) and the batch sweep
        log("config 1 (B = 1) and the batch sweep")
        guarded("config1", lambda: bench_config1(args.precision, dev, args, cpu=not args.no_cpu_baseline))
        guarded("batch_sweep", lambda: bench_batch_sweep(args.precision, dev, args))
    if args.full and rank == 0 and world == 1 and not args.no_other_configs:
        # BASELINE configs[2] / [3] / [4] beside the headline metric (bounded: a few steps each); models of the headline run are released
        torch.cuda.empty_cache()
        for key, what, fn in (("lstm_models", "DisCo / CaMN inference", bench_lstm_models), ("train_step", "one EMAGE training step", bench_train_step)):
            log(f"other BASELINE configs: {what}")
            guarded(key, lambda fn=fn: fn(dev, cpu=not args.no_cpu_baseline))
    if rank == 0:
        print(json.dumps(result), flush=True)
    if hard_exit:
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(0)
    pdist.finalize()


if __name__ == "__main__":
    main()
