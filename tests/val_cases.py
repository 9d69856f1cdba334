"""The case table of the `emage_val_metrics` tests (tests/test_validation_gpu.py, tests/test_validation_host.py): seeded inputs as VIEWS inside
larger tensors whose slack holds valid data (a missing guard shows as a wrong number, never as an access outside an allocation), outputs
inside canary frames, and the bounds the tests assert.

Shapes: M = 130 rows = 26 clips x T = 5 — nine row blocks of 16, the last one ragged.  Three entries, one per tag, with different weights:
  0  K = 256 in a view of leading dimension 300, C = 256 in a view of pitch 260, 16-byte aligned: the 16-byte load paths;
  1  K = 100 and C = 48 in views that start one / two floats into their rows: the one-element paths, widths that are no multiple of 64;
  2  K = 256 aligned, C = 48 misaligned: the two paths mixed in one entry.
Row 3 of entry 0 holds a duplicated maximum (columns 10 and 200); with `poison`, every row at or beyond n_valid * T is NaN in all three
inputs, and row 126 of entry 2 holds a single NaN."""
import torch

from pantomatrix_amd import _lib

CLIPS, T = 26, 5
M = CLIPS * T
SHAPES = ((256, 300, 0, 256, 260, 0), (100, 104, 1, 48, 52, 2), (256, 300, 0, 48, 52, 2))       # K, ld, col0, C, pitch, col0
WEIGHTS = ((1.0, 0.5), (3.0, 0.25), (0.75, 2.0))                                                # l_w, c_w
PAD = 4                                                                                         # slack rows in front of and behind every view
CANARY = -7
SUM_RTOL = 1e-5          # the bound of test_loss_kernels (tests/test_train_forward_gpu.py) for the same two sums
STEP_RTOL = 2e-4         # losses of a whole step against the reference: the bound of test_step_losses_on_device


def build(device, n_valid=CLIPS, poison=True, seed=0, bad_index=False):
    """-> (entries for ops.val_metrics, dict of the framing tensors).  The same seed gives the same valid rows for every n_valid."""
    g = torch.Generator().manual_seed(seed)
    entries, frames = [], dict(pred=[])
    for e, ((k, ld, kc0, c, pitch, cc0), (l_w, c_w)) in enumerate(zip(SHAPES, WEIGHTS)):
        big_x = torch.randn(M + 2 * PAD, ld, generator=g)
        big_r = torch.randn(M + 2 * PAD, pitch, generator=g)
        big_g = torch.randn(M + 2 * PAD, pitch, generator=g)
        x, r, lat = big_x[PAD:PAD + M, kc0:kc0 + k], big_r[PAD:PAD + M, cc0:cc0 + c], big_g[PAD:PAD + M, cc0:cc0 + c]
        idx = torch.randint(0, k, (M,), generator=g)
        idx[::2] = x[::2].argmax(dim=1)                       # every other row is a hit
        if e == 0:
            x[3, 10] = x[3, 200] = x[3].max() + 1.0           # a duplicated maximum: the first one wins
            idx[3] = 10
        if poison:
            rows = n_valid * T
            for t in (x, r, lat):
                t[rows:] = float("nan")
            if e == 2 and n_valid < CLIPS:
                x[M - 4] = torch.randn(k, generator=g)
                x[M - 4, 17] = float("nan")                   # one NaN in an otherwise finite row
        if bad_index and e == 1:
            idx[7] = k                                        # one past the codebook
        big_p = torch.full((M + 2 * PAD,), CANARY, dtype=torch.int64)
        big_x, big_r, big_g, big_p, idx = (t.to(device) for t in (big_x, big_r, big_g, big_p, idx))
        entries.append(dict(rec=big_r[PAD:PAD + M, cc0:cc0 + c], latent=big_g[PAD:PAD + M, cc0:cc0 + c], logits=big_x[PAD:PAD + M, kc0:kc0 + k],
                            index=idx, pred=big_p[PAD:PAD + M], l_w=l_w, c_w=c_w, tag=e))
        frames["pred"].append(big_p)
    return entries, frames


def framed_acc(device):
    """The accumulator block inside a canary frame: (frame, the view to hand to the kernel)."""
    big = torch.full((_lib.VAL_ACC_WORDS + 16,), float(CANARY), dtype=torch.float64, device=device)
    big[8:8 + _lib.VAL_ACC_WORDS] = 0
    return big, big[8:8 + _lib.VAL_ACC_WORDS]


def assert_frames_intact(frames, acc_frame):
    for big_p in frames["pred"]:
        assert bool((big_p[:PAD] == CANARY).all()) and bool((big_p[PAD + M:] == CANARY).all()), "pred_index written outside its view"
    assert bool((acc_frame[:8] == CANARY).all()) and bool((acc_frame[8 + _lib.VAL_ACC_WORDS:] == CANARY).all()), "accumulators written outside their block"


def refused_calls():
    """(what, arguments of emage_val_metrics) for every rule its header lists: each must come back EMAGE_EINVAL before any launch (the
    pointers are made-up addresses that are never dereferenced: every case fails a check)."""
    def table(n=1, **over):
        arr = (_lib.ValEntry * max(n, 1))()
        for e in arr:
            e.rec, e.latent, e.logits, e.index, e.pred = 0x1000, 0x2000, 0x3000, 0x4000, None
            e.ld_rec, e.ld_latent, e.ld_logits, e.C, e.K, e.pred_rows, e.tag, e.pred_ld, e.l_w, e.c_w = 48, 48, 100, 48, 100, 0, 0, 0, 1.0, 1.0
            for k, v in over.items():
                setattr(e, k, v)
        return arr

    nv, acc, ws, big = 0x5000, 0x6000, 0x7000, 1 << 30
    good = dict(n=1, m=M, t=T, n_valid=nv, acc=acc, ws=ws, ws_bytes=big)
    cases = [("no entries", None, {}), ("no n_valid", table(), dict(n_valid=None)), ("no accumulators", table(), dict(acc=None)),
             ("no workspace", table(), dict(ws=None)), ("workspace too small", table(), dict(ws_bytes=8)),
             ("M % T != 0", table(), dict(t=4)), ("T <= 0", table(), dict(t=0)), ("M <= 0", table(), dict(m=0)),
             ("13 entries", table(13), dict(n=13)), ("0 entries", table(), dict(n=0)),
             ("K = 1", table(K=1), {}), ("K = 1025", table(K=1025, ld_logits=2048), {}), ("C = 0", table(C=0), {}), ("C = 1025", table(C=1025, ld_rec=2048, ld_latent=2048), {}),
             ("ld_rec < C", table(ld_rec=47), {}), ("ld_latent < C", table(ld_latent=47), {}), ("ld_logits < K", table(ld_logits=99), {}),
             ("tag 3", table(tag=3), {}), ("pred view does not divide M", table(pred=0x8000, pred_rows=7, pred_ld=7), {}),
             ("pred pitch < rows", table(pred=0x8000, pred_rows=T, pred_ld=T - 1), {})]
    for name in ("rec", "latent", "logits", "index"):
        cases.append((f"no {name}", table(**{name: None}), {}))
    out = []
    for what, arr, over in cases:
        a = dict(good, **over)
        out.append((what, (arr, a["n"], a["m"], a["t"], a["n_valid"], a["acc"], a["ws"], a["ws_bytes"], None)))
    return out
