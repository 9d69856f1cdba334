"""Generate tests/golden/train_step_speakers.npz from the REAL reference training step (train_emage_audio.py:132-180 run through
oracle/reference_harness.reference_train_step) with SEVERAL speakers — build container only (the reference tree).
    python tests/golden/make_golden_train_speakers.py
speaker_dims = 4, batch 4, ids [2, 0, 2, 1]: row 2 is fed by two clips that are not neighbours, row 3 by none.  The reference's
train_val_fn builds `speaker_id = zeros` itself (T:146), so a forward pre-hook on the reference model replaces that one argument and the
step is otherwise the reference's own, called unchanged.  The fixture holds what train_step_b2.npz holds plus the FULL gradients of the
two speaker tables and their values after Adam (whole-tensor norms cannot see two rows swapped)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import common  # noqa: E402
from oracle import reference_harness as rh  # noqa: E402
from tools.workloads import train_batch  # noqa: E402

ITERATION, SEED = 0, 11
SPEAKER_DIMS, SPEAKER_IDS = 4, (2, 0, 2, 1)
TABLES = ("speaker_embedding_body.weight", "speaker_embedding_face.weight")


def main():
    assert rh.available(), "needs the reference tree"
    acfg, vqc, gc = common.cfg_dicts()
    acfg = dict(acfg, speaker_dims=SPEAKER_DIMS)
    bs = len(SPEAKER_IDS)
    model, vq = rh.build_reference(acfg, vqc, gc, 0)
    ids = torch.tensor(SPEAKER_IDS, dtype=torch.long).reshape(bs, 1)
    calls = []

    def with_ids(_module, args, kwargs):                 # model(audio, speaker_id, masked_motion=..., mask=..., use_audio=...) (T:156-171)
        assert args[1].shape == ids.shape and not args[1].any()
        calls.append(1)
        return (args[0], ids.to(args[1].device), *args[2:]), kwargs

    handle = model.register_forward_pre_hook(with_ids, with_kwargs=True)
    try:
        losses, grads, sd_after = rh.reference_train_step(model, vq, acfg, train_batch(bs=bs), ITERATION, SEED)
    finally:
        handle.remove()
    assert len(calls) == 3
    names = sorted(grads)
    gmax = max(float(g.abs().max()) for g in grads.values())
    total = float(torch.sqrt(sum(g.double().pow(2).sum() for g in grads.values())))
    out = {"iteration": ITERATION, "seed": SEED, "bs": bs, "speaker_dims": SPEAKER_DIMS, "speaker_ids": np.array(SPEAKER_IDS, dtype=np.int64),
           "grad_names": np.array(names),
           "grad_norms": np.array([float(grads[n].norm()) for n in names]),
           "grad_first": np.array([float(grads[n].reshape(-1)[0]) for n in names]),
           "shadowed": np.array([float(grads[n].abs().max()) < 1e-5 * gmax for n in names]),
           "param_sum_after": np.array([float(sd_after[n].double().sum()) for n in names]),
           "total_grad_norm": total}
    for n in TABLES:
        out["grad/" + n] = grads[n].numpy()
        out["after/" + n] = sd_after[n].numpy()
    for k, v in losses.items():
        out["loss_" + k] = v
    path = os.path.join(HERE, "train_step_speakers.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, {k: round(v, 5) for k, v in losses.items()}, "params with grad:", len(names), "shadowed:", int(out["shadowed"].sum()),
          "total gradient norm:", round(total, 4), "row norms:", {n: [round(float(r.norm()), 6) for r in grads[n]] for n in TABLES})


if __name__ == "__main__":
    main()
