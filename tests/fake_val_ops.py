"""TEST-ONLY CPU stand-in of `ops.val_metrics` (include/emage_hip.h: emage_val_metrics), in the manner of tests/fake_clip_ops.py:
`installed()` is `fake_clip_ops.installed()` plus the kernel's CONTRACT restated with torch on host tensors, so `validation.Validator` and the
evaluation loader run without a GPU.  `val_metrics_reference` is the same contract in float64 on numpy copies — the oracle of the GPU
kernel tests (tests/val_cases.py builds its inputs).  Calls are recorded in `fake_ops.CALLS` as "val_metrics"."""
import contextlib

import numpy as np
import torch

import fake_clip_ops
import fake_ops
from pantomatrix_amd import _lib, ops

NEW_CALLS = ("val_metrics",)


def val_metrics_reference(entries, t, n_valid):
    """The per-batch values of emage_val_metrics in float64 from the same fp32 inputs: -> dict(last (7,), hits [per entry], rows, bad,
    pred [per entry: the arg-max of the float64 log-softmax over ALL rows, first maximum on ties]).  Rows at or beyond n_valid * t are
    left out of every sum; the MSE takes difference and square in fp32 (as the kernel and torch's mse_loss do) and sums in float64."""
    m = entries[0]["rec"].shape[0]
    rows = max(0, min(int(n_valid), m // t)) * t
    last, hits, preds, bad = np.zeros(_lib.VAL_LOSSES), [], [], 0
    for e in entries:
        x = e["logits"].detach().cpu().numpy().astype(np.float64)
        with np.errstate(all="ignore"):
            mx = np.nanmax(np.where(np.isnan(x), -np.inf, x), axis=1, keepdims=True)
            lsm = (x - mx) - np.log(np.exp(x - mx).sum(axis=1, keepdims=True))
        preds.append(np.argmax(np.where(np.isnan(lsm), np.inf, lsm), axis=1))
        idx = e["index"].detach().cpu().numpy().reshape(-1)
        k = x.shape[1]
        ok = (idx[:rows] >= 0) & (idx[:rows] < k)
        bad |= int((~ok).any()) if rows else 0
        r = np.arange(rows)[ok]
        nll = float(-lsm[r, idx[:rows][ok]].sum()) if rows else 0.0
        hits.append(int((preds[-1][r] == idx[:rows][ok]).sum()) if rows else 0)
        d = (e["rec"].detach().cpu().numpy()[:rows] - e["latent"].detach().cpu().numpy()[:rows]).astype(np.float32)
        mse = float((d * d).astype(np.float64).sum())
        if rows:
            last[2 * e["tag"]] += float(e["l_w"]) * mse / (rows * d.shape[1])
            last[2 * e["tag"] + 1] += float(e["c_w"]) * nll / rows
    last[6] = last[:6].sum()
    return dict(last=last, hits=hits, rows=rows, bad=bad, pred=preds)


def val_metrics(entries, t, n_valid, acc, workspace=None):
    """emage_val_metrics as its header states it, on host tensors: fp32 log-softmax, the arg-max of `fake_ops.argmax_logsoftmax`, sums over
    the first n_valid * t rows only, `pred` written for every row, nothing changed by an empty batch."""
    fake_ops.CALLS.append("val_metrics")
    assert 1 <= len(entries) <= _lib.VAL_MAX_ENTRIES and n_valid.dtype == torch.int32 and n_valid.numel() == 1
    assert acc.dtype == torch.float64 and acc.numel() == _lib.VAL_ACC_WORDS
    m = entries[0]["rec"].shape[0]
    assert m % t == 0
    rows = max(0, min(int(n_valid), m // t)) * t
    last, hits, bad = [0.0] * _lib.VAL_LOSSES, [], 0
    for e in entries:
        assert e["rec"].shape == e["latent"].shape and e["logits"].shape[0] == m and e["index"].numel() == m and 0 <= e["tag"] < _lib.VAL_TAGS
        lsm = torch.log_softmax(e["logits"].float(), dim=1)
        pred = torch.max(lsm, dim=1)[1]
        if e.get("pred") is not None:
            e["pred"].copy_(pred.view(e["pred"].shape))
        idx = e["index"].reshape(-1)[:rows]
        ok = (idx >= 0) & (idx < lsm.shape[1])
        bad |= int((~ok).any()) if rows else 0
        r = torch.arange(rows)[ok]
        nll = float(-lsm[r, idx[ok]].double().sum())
        hits.append(int((pred[r] == idx[ok]).sum()))
        d = e["rec"][:rows].float() - e["latent"][:rows].float()
        mse = float((d * d).double().sum())
        if rows:
            last[2 * e["tag"]] += float(e["l_w"]) * (mse / (rows * d.shape[1]))
            last[2 * e["tag"] + 1] += float(e["c_w"]) * (nll / rows)
    if rows == 0:
        return workspace
    last[6] = sum(last[:6])
    ints = acc.view(torch.int64)
    for k, v in enumerate(last):
        acc[_lib.VAL_ACC_LAST + k] = v
        acc[_lib.VAL_ACC_METER + k] += v
    for e, h in enumerate(hits):
        ints[_lib.VAL_ACC_HITS + e] += h
        ints[_lib.VAL_ACC_LAST_HITS + e] = h
    ints[_lib.VAL_ACC_ROWS] += rows
    ints[_lib.VAL_ACC_LAST_ROWS] = rows
    ints[_lib.VAL_ACC_BATCHES] += 1
    if bad:
        ints[_lib.VAL_ACC_STATUS] |= 1
    return workspace


@contextlib.contextmanager
def installed():
    with fake_clip_ops.installed():
        saved = ops.val_metrics
        try:
            ops.val_metrics = val_metrics
            yield
        finally:
            ops.val_metrics = saved
