#!/usr/bin/env python
"""Forward side of the EMAGE training step at BASELINE config 3 (per-GPU batch 56 x 64-frame clips) on the MI355X:
targets through the HIP VQ models, the three train-mode forwards (batch-statistics BatchNorm, dropout with device-drawn
masks) and the six losses (pantomatrix_amd/training.py).  Eager launches, one stream.  Prints one JSON line.
--full-step --graph --speakers N: the captured step of a model with `speaker_dims = N` and mixed per-clip ids (clip i speaks as i mod N;
the two embedding gradients go through `emage_embedding_backward`) NEXT TO the one-speaker step in the same call: `--runs` alternating
runs of `--steps` replays per arm -> per arm the runs, their median and spread, and the calls into the library of one eager step by
operator name (`emage_op_calls`: the two arms differ in the six embedding gradients only)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402


def draw_masks(b, t, d, ff, h, ta, dev, p=0.1):
    from pantomatrix_amd import spec
    mk = lambda *shape: (torch.rand(*shape, device=dev) >= p).float() / (1 - p)
    dec = lambda tk: [mk(b, h, t, t), mk(t, b, d), mk(b, h, t, tk), mk(t, b, d), mk(t, b, ff), mk(t, b, d)]
    enc = [mk(b, h, t, t), mk(t, b, d), mk(t, b, ff), mk(t, b, d)]
    out = [mk(b, t, d)]
    for _ in range(spec.N_FACE_LAYERS):
        out += dec(t)
    out += [mk(b, t, d)] + enc + [mk(b, t, d)]
    for _ in range(spec.N_CROSS_LAYERS):
        out += dec(ta)
    for _ in range(3):
        out += dec(t)
    return out


def _batch(b, t, dev):
    g = torch.Generator().manual_seed(5)
    batch = dict(motion=0.3 * torch.randn(b, t, 165, generator=g), audio=0.1 * torch.randn(b, t * 16000 // 30, generator=g),
                 expressions=0.5 * torch.randn(b, t, 100, generator=g), trans=0.1 * torch.randn(b, t, 3, generator=g),
                 foot_contact=(torch.rand(b, t, 4, generator=g) > 0.5).float())
    return {k: v.to(dev) for k, v in batch.items()}


class _CallsByName:
    """The measurement hook of `ops` (`_TRACE`): the operator calls that reach the library, by operator."""

    def __init__(self):
        import collections
        self.calls = collections.Counter()

    def tag(self):
        return None

    def fire(self, kind, entries, launch):
        self.calls[kind] += 1
        return launch()


def speakers_ab(args):
    """The captured step with one speaker row against the one with `--speakers` rows and mixed ids, alternating in one process."""
    import statistics

    import common
    import pantomatrix_amd as pa
    from pantomatrix_amd import ops, synthetic, training
    dev, b, t = "cuda", args.batch, 64
    batch = _batch(b, t, dev)
    random_mask = (torch.rand(b, t, 337, device=dev) < 0.5).float()
    one, vq = common.product_models(precision=args.precision, device=dev)
    cfg = pa.EmageAudioConfig(**dict(common.cfg_dicts()[0], speaker_dims=args.speakers))
    many = pa.EmageAudioModel(cfg)
    many.load_state_dict(synthetic.audio_model_state(cfg, 0))
    many.set_precision(args.precision)
    many.to(dev).eval()
    ids = (torch.arange(b, device=dev) % args.speakers).reshape(b, 1)
    arms = {"one_speaker": (one, None), f"{args.speakers}_speakers": (many, ids)}
    trainers, calls = {}, {}
    for name, (model, spk) in arms.items():
        tr = training.Trainer(model, vq, max_grad_norm=args.max_grad_norm)
        tr.step(batch, random_mask=random_mask, speaker_id=spk)       # lazy initialisation, the exchange schedule
        counter = _CallsByName()
        ops._TRACE[0] = counter
        try:
            tr.step(batch, random_mask=random_mask, speaker_id=spk)
        finally:
            ops._TRACE[0] = None
        calls[name] = dict(sorted(counter.calls.items()))
        trainers[name] = tr.capture(batch, random_mask, speaker_id=spk)
    for _ in range(3):                                               # both graphs warm (the second capture follows the first arm's set-up)
        for tr in trainers.values():
            tr.replay()
    torch.cuda.synchronize()
    ms = {name: [] for name in arms}
    for _ in range(args.runs):
        for name, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _s in range(args.steps):
                losses = tr.replay()
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - t0) / args.steps)
    a, c = calls["one_speaker"], calls[f"{args.speakers}_speakers"]
    print(json.dumps({"what": "one whole EMAGE optimisation step as ONE hipGraph replay, one speaker row against several with mixed per-clip ids, "
                              "alternating runs in one process",
                      "config": {"workload": "BASELINE config 3", "clips_per_gpu": b, "frames_per_clip": t, "speaker_dims": args.speakers,
                                 "steps_per_run": args.steps, "runs": args.runs}, "dtype": args.precision, "max_grad_norm": args.max_grad_norm,
                      "ms_per_step": {k: {"runs": [round(x, 3) for x in v], "median": round(statistics.median(v), 3), "spread": round(max(v) - min(v), 3)}
                                      for k, v in ms.items()},
                      "emage_op_calls": {k: sum(v.values()) for k, v in calls.items()},
                      "emage_op_calls_that_differ": {k: [a.get(k, 0), c.get(k, 0)] for k in sorted(set(a) | set(c)) if a.get(k, 0) != c.get(k, 0)},
                      "peak_memory_gb": torch.cuda.max_memory_allocated() / 2 ** 30, "losses": {k: round(v, 4) for k, v in losses.items()}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=56)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--graph", action="store_true", help="with --full-step: the step captured as one hipGraph (Trainer.capture / replay; precision fp32)")
    ap.add_argument("--full-step", action="store_true", help="whole optimisation steps (training.Trainer.step: + backward, Adam) instead of the forward side")
    ap.add_argument("--max-grad-norm", type=float, default=None, help="with --full-step: clip the gradient by its global norm inside the step "
                    "(training.Trainer(max_grad_norm=...); the reference's configs/emage_audio.yaml has 0.99)")
    ap.add_argument("--speakers", type=int, default=None, help="with --full-step --graph: also time the step of a model with this many speaker rows "
                    "and mixed per-clip ids, alternating with the one-speaker step")
    ap.add_argument("--runs", type=int, default=3, help="with --speakers: alternating runs per arm")
    args = ap.parse_args()
    if args.speakers is not None:
        if not (args.full_step and args.graph) or args.speakers < 2:
            ap.error("--speakers N (N >= 2) needs --full-step --graph")
        return speakers_ab(args)
    import common
    from pantomatrix_amd import training
    dev = "cuda"
    model, vq = common.product_models(precision=args.precision, device=dev)
    fwd = training.TrainForward(model)
    b, t = args.batch, 64
    batch = _batch(b, t, dev)
    c = model.config
    ta = model._wav_lengths(batch["audio"].shape[1])[-1]
    random_mask = (torch.rand(b, t, 337, device=dev) < 0.5).float()

    if args.max_grad_norm is not None and not args.full_step:
        ap.error("--max-grad-norm needs --full-step")
    trainer = training.Trainer(model, vq, max_grad_norm=args.max_grad_norm) if args.full_step else None
    if args.graph:
        trainer.capture(batch, random_mask)                          # dropout masks are drawn inside the graph (ops.dropout_mask)

        def step():
            return trainer.replay(), None
    else:
        step = None

    def eager_step():
        masks = [draw_masks(b, t, c.hidden_size, 2 * c.hidden_size, 4, ta, dev) for _ in range(3)]
        if trainer is not None:
            return trainer.step(batch, 0, masks, random_mask), None
        return training.step_losses(fwd, vq, batch, 0, masks, random_mask)

    step = step or eager_step
    step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        losses, _ = step()
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / args.steps
    what = ("one whole EMAGE optimisation step (targets, 3 x (train-mode forward, losses, backward), Adam), "
            + ("ONE hipGraph replay (+ drawing the dropout masks)" if args.graph else "eager, one stream") + "; f16x3: split-fp16 MFMA "
            "contractions forward and backward, fp32: exact-fp32 MFMA" if args.full_step else
            "forward side of one EMAGE training step (targets + 3 train-mode forwards + 6 losses), eager, one stream")
    print(json.dumps({"what": what, "config": {"workload": "BASELINE config 3", "clips_per_gpu": b, "frames_per_clip": t}, "dtype": args.precision,
                      "max_grad_norm": args.max_grad_norm, "ms_per_step": ms, "clip_windows_per_s": b / (ms * 1e-3), "peak_memory_gb": torch.cuda.max_memory_allocated() / 2 ** 30,
                      "losses": {k: round(v, 4) for k, v in losses.items()}}))


if __name__ == "__main__":
    main()
