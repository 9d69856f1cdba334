"""Generate tests/golden/vq_train_step.npz from the REAL reference tokenizer classes (EmageVQVAEConv / EmageVAEConv of
the reference's models/emage_audio, imported read-only on the CPU through oracle/reference_harness.py) — where the reference is present only.
    python tests/golden/make_golden_vq_train.py
Per case of tests/vq_train_common.py (a 2-layer and a 3-layer VQ tokenizer of different widths, the global VAE): seeded synthetic
weights, `model.train()`, ONE forward, loss = mse(rec_pose, x) + embedding_loss, backward, ONE torch.optim.Adam step.  Recorded:
the codes, the loss, every parameter's gradient norm / first element / largest magnitude, the FULL codebook gradient (256 x 256: the one
tensor the new kernels own; its unused rows are zero and compress away), the parameter sums after the update, the two scalars, and every
ROW_STEP-th row of rec_pose / poses_feat.  Inputs are NOT stored (as in make_golden.py): tests regenerate them from the same seed
(tests/vq_train_common.py::case_input); their float64 sum is recorded as a check.  That keeps the fixture near 150 KB.  The reference has no tokenizer trainer: this is the minimal objective the product's
`TokenizerTrainer` runs, computed by the reference's own modules and torch autograd."""
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import vq_train_common as vc  # noqa: E402
from oracle import reference_harness as rh  # noqa: E402


def run_case(ref, tag):
    kind = vc.CASES[tag][0]
    cfg = vc.case_config(tag)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = ref.EmageVQVAEConv(ref.EmageVQVAEConvConfig(**cfg)) if kind == "vq" else ref.EmageVAEConv(ref.EmageVAEConvConfig(**cfg))
    model.load_state_dict(vc.case_state(tag), strict=True)
    for p in model.parameters():
        p.requires_grad = True
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=vc.LR, betas=vc.BETAS, eps=vc.EPS, weight_decay=0.0)
    x = vc.case_input(tag)
    out = model(x)
    loss = F.mse_loss(out["rec_pose"], x)
    rows = lambda t: t.detach().reshape(-1, t.shape[-1])[::vc.ROW_STEP].numpy()
    rec = {f"{tag}_x_sum": float(x.double().sum()), f"{tag}_rec_pose_rows": rows(out["rec_pose"]), f"{tag}_rec_loss": float(loss.detach())}
    if kind == "vq":
        loss = loss + out["embedding_loss"]
        with torch.no_grad():
            idx = model.quantizer.map2index(model.encoder(x)).reshape(-1)
        counts = torch.bincount(idx, minlength=cfg["vae_codebook_size"])
        # a condition on the DATA: codes repeat, some heavily, and some codes stay unused (their gradient rows must be exactly zero)
        assert int((counts == 0).sum()) >= 1 and int(counts.max()) > 8, (tag, int((counts == 0).sum()), int(counts.max()))
        rec.update({f"{tag}_idx": idx.numpy().astype(np.int16), f"{tag}_poses_feat_rows": rows(out["poses_feat"]),
                    f"{tag}_embedding_loss": float(out["embedding_loss"].detach()), f"{tag}_perplexity": float(out["perplexity"].detach())})
        print(tag, "codes used:", int((counts > 0).sum()), "max count:", int(counts.max()), "perplexity:", float(out["perplexity"].detach()))
    loss.backward()
    names = [n for n, p in model.named_parameters() if p.grad is not None]
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    opt.step()
    after = dict(model.named_parameters())
    rec.update({f"{tag}_loss": float(loss.detach()), f"{tag}_grad_names": np.array(names),
                f"{tag}_grad_norms": np.array([float(grads[n].norm()) for n in names]),
                f"{tag}_grad_first": np.array([float(grads[n].reshape(-1)[0]) for n in names]),
                f"{tag}_grad_absmax": np.array([float(grads[n].abs().max()) for n in names]),
                f"{tag}_param_sum_after": np.array([float(after[n].detach().double().sum()) for n in names])})
    if kind == "vq":
        rec[f"{tag}_grad_codebook"] = grads["quantizer.embedding.weight"].numpy()
    print(tag, "loss", float(loss.detach()), "params with grad:", len(names))
    return rec


def main():
    assert rh.available(), "needs the reference checkout (oracle/reference_harness.py)"
    ref = rh.import_reference()
    out = {"lr": vc.LR, "row_step": vc.ROW_STEP}
    for tag in vc.CASES:
        out.update(run_case(ref, tag))
    path = os.path.join(HERE, "vq_train_step.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
