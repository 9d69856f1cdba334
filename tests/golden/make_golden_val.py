"""Generate tests/golden/val_step.npz from the REAL reference validation step (train_emage_audio.py:130-204 with mode="val", run
through oracle/reference_harness.reference_train_functions) — build container only (the reference tree).
    python tests/golden/make_golden_val.py
The fixture pins what `validation.Validator` is compared with on machines without the reference: the seven losses of a 3-clip batch and of
its first two clips (the SAME random mask on those clips: the partial-batch tests), the mask, per forward and part the arg-max codes, the
hit counts and the rows whose top-2 logit margin is below MARGIN (left out of cross-implementation code comparisons; at most CAP of all
rows, asserted here), and the decoded rot-6D of the first clip as handed to `fgd_evaluator.update`."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import common  # noqa: E402
from oracle import reference_harness as rh  # noqa: E402

ITERATION, SEED, BS = 0, 11, 3
MARGIN, CAP = 1e-3, 0.01
TAGS = ("seed", "audio", "mask")
PARTS = ("face", "upper", "hands", "lower")
LOSS_KEYS = ("rec_seed", "cls_seed", "rec_audio", "cls_audio", "rec_mask", "cls_mask", "all")


class _Evaluator:
    def __init__(self):
        self.calls = []

    def update(self, pred, gt):
        self.calls.append((pred.detach().clone(), gt.detach().clone()))


class _TorchWithMask:
    """`torch` as train_val_fn sees it, with `rand` returning a given tensor: the 2-clip run takes the 3-clip run's mask on its clips."""

    def __init__(self, rand):
        self._rand = rand

    def __getattr__(self, name):
        return getattr(torch, name)

    def rand(self, *shape):
        assert tuple(shape) == tuple(self._rand.shape), (shape, self._rand.shape)
        return self._rand


def run(model, vq, acfg, batch, rand):
    """-> (losses, per-forward model outputs, (pred, gt) handed to the evaluator, the reference's index targets)."""
    fns = rh.reference_train_functions()
    fns["torch"] = _TorchWithMask(rand)
    cfg = types.SimpleNamespace(model=types.SimpleNamespace(**acfg), solver=types.SimpleNamespace(max_grad_norm=0.99))
    outs, ev = [], _Evaluator()
    hook = model.register_forward_hook(lambda _m, _a, out: outs.append({k: v.detach().clone() for k, v in out.items()}))
    try:
        with torch.no_grad():
            losses = fns["train_val_fn"](cfg, batch, model, torch.device("cpu"), mode="val", motion_vq=vq, ClsFn=torch.nn.NLLLoss(),
                                         iteration=ITERATION, fgd_evaluator=ev)
            index = vq.map2index(ev.calls[0][1], batch["expressions"], tar_contact=batch["foot_contact"], tar_trans=batch["trans"])
    finally:
        hook.remove()
    assert len(outs) == 3 and len(ev.calls) == 1
    return {k: float(v) for k, v in losses.items()}, outs, ev.calls[0], index


def codes_of(outs, index):
    codes, small, hits = {}, {}, {}
    for f, tag in enumerate(TAGS):
        for p in PARTS:
            logits = outs[f][f"cls_{p}"]
            lsm = torch.log_softmax(logits, dim=2)
            code = torch.max(lsm, dim=2)[1]
            top2 = torch.topk(logits, 2, dim=2)[0]
            codes[f"{tag}_{p}"] = code.numpy().astype(np.int16)
            small[f"{tag}_{p}"] = ((top2[..., 0] - top2[..., 1]) < MARGIN).numpy()
            hits[f"{tag}_{p}"] = int((code == index[p]).sum())
    return codes, small, hits


def main():
    assert rh.available(), "needs the reference tree"
    acfg, vqc, gc = common.cfg_dicts()
    model, vq = rh.build_reference(acfg, vqc, gc, 0)
    batch = common.train_batch(bs=BS)
    rand = torch.rand(BS, batch["motion"].shape[1], acfg["pose_dims"] + 7, generator=torch.Generator().manual_seed(SEED))
    out = {"iteration": ITERATION, "seed": SEED, "bs": BS, "margin": MARGIN,
           "random_mask": np.packbits((rand < (ITERATION / 135 * 400) * 0.95 + 0.05).numpy().reshape(-1))}
    for n in (BS, BS - 1):
        losses, outs, (pred, _gt), index = run(model, vq, acfg, {k: v[:n] for k, v in batch.items()}, rand[:n])
        codes, small, hits = codes_of(outs, index)
        rows = sum(v.size for v in small.values())
        under = sum(int(v.sum()) for v in small.values())
        assert under <= CAP * rows, (under, rows)
        out[f"losses_b{n}"] = np.array([losses[k] for k in LOSS_KEYS])
        out[f"hits_b{n}"] = np.array([hits[f"{t}_{p}"] for t in TAGS for p in PARTS], dtype=np.int64)
        for key in codes:
            out[f"codes_b{n}_{key}"] = codes[key]
            out[f"small_b{n}_{key}"] = np.packbits(small[key].reshape(-1))
        if n == BS:
            out["decoded_clip0"] = pred[0].numpy().astype(np.float32)
        print(f"bs {n}:", {k: round(v, 4) for k, v in losses.items()}, f"rows under the margin: {under} of {rows}")
    path = os.path.join(HERE, "val_step.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
