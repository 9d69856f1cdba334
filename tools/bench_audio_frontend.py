#!/usr/bin/env python
"""What the audio front end costs on the host and on the device (run on the MI355X).  One JSON line (also written to --out).

Workloads: the EMAGE batch (64 clips x 128 frames = 68 267 samples at 16 kHz) and the CaMN batch (256 clips x 28 s), each arriving as
44.1 kHz stereo int16 and as 48 kHz mono int16.

* host:   what `motion_io.load_audio` does per clip — decode the int16 bytes, channel mean, `scipy.signal.resample_poly` in float64, float32 —
          over the batch on 16 worker processes (forked before the device is touched).  --host-clips N times the first N clips of a batch
          and scales to the batch (reported as such); 0 = the whole batch.
* device: `ops.audio_resample` on the same PCM: device events around `--iters` launches in a row after a warm-up, `--windows` such windows
          (minimum and median reported), rotating over enough distinct input / output buffers that a launch's 'PCM in + fp32 out' bytes
          cannot stay in the 256 MiB Infinity Cache; those bytes over the time, as a share of the 8 TB/s HBM peak (AMD's MI355X data sheet).
          A launch-to-launch time between events includes the launch gap; `rocprofv3 --kernel-trace --stats -- python tools/bench_audio_frontend.py
          --no-runner` gives the kernel's own time (kernel name `audio_resample_kernel`) in a run of its own.
* runner: the captured EMAGE step (64 clips) of `ClipRunner` on 16 kHz float audio and of `ClipRunner(audio_input=44.1 kHz stereo)`,
          alternated, against the launch's own time.
    python tools/bench_audio_frontend.py [--iters 200] [--windows 5] [--host-clips 32] [--no-runner] [--out profiles/audio_frontend.json]"""
import argparse
import json
import multiprocessing as mp
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pantomatrix_amd import audio, synthetic  # noqa: E402

HBM_PEAK = 8.0e12                              # bytes / s: the data-sheet peak of the MI355X's HBM3E
WORKERS = 16
_PCM = None                                    # the batch the forked workers read


def pcm_batch(clips, n_in, ch, seed):
    rng = np.random.default_rng(seed)
    one = np.clip(np.rint(0.1 * 32768 * rng.standard_normal((8, n_in, ch))), -32768, 32767).astype(np.int16)
    return one[np.arange(clips) % 8]           # 8 distinct clips repeated: the timing does not depend on the values


def _host_clip(args):
    i, up, down = args
    from scipy.signal import resample_poly
    raw = _PCM[i].tobytes()                     # a file's `data` chunk
    x = np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0
    x = x.reshape(-1, _PCM.shape[2])
    x = x.mean(axis=1) if x.shape[1] > 1 else x[:, 0]
    return resample_poly(x.astype(np.float64), up, down).astype(np.float32)


def host_seconds(pcm, up, down, clips):
    global _PCM
    _PCM = pcm
    with mp.get_context("fork").Pool(WORKERS) as pool:
        pool.map(_host_clip, [(i, up, down) for i in range(min(WORKERS, clips))])       # start the workers, import scipy
        t0 = time.perf_counter()
        out = pool.map(_host_clip, [(i, up, down) for i in range(clips)], chunksize=1)
        dt = time.perf_counter() - t0
    return dt, out[0]


def device_seconds(torch, pcm_host, ch, rate, iters, windows):
    from pantomatrix_amd import ops
    dev = torch.device("cuda", 0)
    b, n_in = pcm_host.shape[:2]
    n_out = audio.out_length(n_in, *audio.rate_ratio(rate, 16000))
    moved = pcm_host.nbytes + b * n_out * 4
    copies = max(2, min(8, -(-(320 << 20) // moved)))
    ins = [torch.from_numpy(pcm_host).to(dev) for _ in range(copies)]
    outs = [torch.empty(b, n_out, dtype=torch.float32, device=dev) for _ in range(copies)]
    for i in range(3):
        ops.audio_resample(ins[i % copies], ch, rate, out=outs[i % copies])
    torch.cuda.synchronize()
    secs = []
    for _ in range(windows):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for i in range(iters):
            ops.audio_resample(ins[i % copies], ch, rate, out=outs[i % copies])
        stop.record()
        torch.cuda.synchronize()
        secs.append(start.elapsed_time(stop) * 1e-3 / iters)
    return secs, moved, copies, outs[0][0].cpu().numpy()


def runner_times(torch, steps):
    from pantomatrix_amd.runtime import ClipRunner
    from tools import workloads as common
    dev = torch.device("cuda", 0)
    model, vq = common.product_models(precision="f16x3", device=dev)
    n = synthetic.samples_for_frames(128)
    spec = audio.AudioInput(44100, 2, "s16")
    pcm = torch.from_numpy(pcm_batch(64, spec.frames_for(n), 2, seed=1)).to(dev)
    fed = ClipRunner(model, vq, 64, n, audio_input=spec)
    plain = ClipRunner(model, vq, 64, n)
    fed.run_device(pcm)
    plain.run_device(fed.audio)                # the same waveform: the two graphs differ by the front-end launch only
    torch.cuda.synchronize()
    same = all(torch.equal(a, b) for a, b in zip(fed.out, plain.out))
    ms = {"float_16k": [], "pcm_44k1_stereo": []}
    for _ in range(3):
        for key, r in (("float_16k", plain), ("pcm_44k1_stereo", fed)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                r.run_device()
            torch.cuda.synchronize()
            ms[key].append(1e3 * (time.perf_counter() - t0) / steps)
    return {"steps_per_round": steps, "ms_per_step_rounds": ms, "ms_per_step_best": {k: min(v) for k, v in ms.items()}, "outputs_equal": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--host-clips", type=int, default=32)
    ap.add_argument("--no-runner", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    work = [("emage_64x128f", 64, synthetic.samples_for_frames(128)), ("camn_256x28s", 256, 28 * 16000)]
    inputs = [("44k1_stereo_s16", 44100, 2), ("48k_mono_s16", 48000, 1)]
    res = {"host_workers": WORKERS, "hbm_peak_bytes_per_s": HBM_PEAK, "iters_per_window": a.iters, "windows": a.windows, "cases": {}}
    batches = {}
    for wname, clips, n_samples in work:                        # the host side first: the workers are forked before the device is opened
        for iname, rate, ch in inputs:
            up, down = audio.rate_ratio(rate, 16000)
            n_in = audio.AudioInput(rate, ch).frames_for(n_samples)
            pcm = pcm_batch(clips, n_in, ch, seed=rate)
            timed = clips if a.host_clips <= 0 else min(clips, a.host_clips)
            dt, first = host_seconds(pcm, up, down, timed)
            batches[wname, iname] = (pcm, rate, ch, first)
            res["cases"][f"{wname}/{iname}"] = {"clips": clips, "frames_in": n_in, "samples_out": audio.out_length(n_in, up, down),
                                                "host": {"clips_timed": timed, "seconds_timed": dt, "ms_per_batch": 1e3 * dt * clips / timed,
                                                         "scaled": timed != clips}}
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_audio_frontend: needs an MI355X (the device side has no CPU path)")
    for (wname, iname), (pcm, rate, ch, first) in batches.items():
        secs, moved, copies, dev_first = device_seconds(torch, pcm, ch, rate, a.iters if pcm.nbytes < (1 << 29) else max(4, a.iters // 10), a.windows)
        sec = min(secs)
        c = res["cases"][f"{wname}/{iname}"]
        c["device"] = {"us_per_launch": 1e6 * sec, "us_per_launch_median": 1e6 * float(np.median(secs)), "us_per_launch_windows": [1e6 * s for s in secs],
                       "bytes_moved": moved, "buffers_rotated": copies, "tbytes_per_s": moved / sec / 1e12,
                       "share_of_hbm_peak": moved / sec / HBM_PEAK, "time_over_floor": sec * HBM_PEAK / moved,
                       "floor_us_at_hbm_peak": 1e6 * moved / HBM_PEAK, "max_abs_diff_vs_host": float(np.abs(dev_first - first).max())}
        c["host_over_device"] = c["host"]["ms_per_batch"] * 1e-3 / sec
    if not a.no_runner:
        res["clip_runner_emage_64"] = runner_times(torch, 20)
        launch = res["cases"]["emage_64x128f/44k1_stereo_s16"]["device"]["us_per_launch"] * 1e-3
        best = res["clip_runner_emage_64"]["ms_per_step_best"]
        res["clip_runner_emage_64"]["front_end_launch_ms"] = launch
        res["clip_runner_emage_64"]["pcm_minus_float_ms"] = best["pcm_44k1_stereo"] - best["float_16k"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
