"""The host arithmetic of the autoregressive windows of `inference()` (M:343-470), once: how a length splits into full windows and a tail,
the lock-step schedule of several lengths, samples per frame, the identity seed.  `modeling_emage_audio` (the window loop and
`_window_step`), `recordings` and `streaming` all read it from here; it imports none of them."""
from __future__ import annotations

import torch

from .data import SMPLX_FPS

MODEL_SR = 16000                                        # `inference()` hard-codes 16000 // 30 samples per frame (M:345, M:393)
SPF = MODEL_SR // SMPLX_FPS
SEED_DIMS = 337                                         # 55 joints x 6, trans, foot contact (T:59-60)


def frames_of(n_samples):
    """M:345."""
    return int(n_samples) * SMPLX_FPS // MODEL_SR


def split_length(frames, window=64, seed_frames=4):
    """One length -> (rounds, remain, tail_frames), M:364-368 / M:428-431: `rounds = (T - seed) // (window - seed)` full windows,
    `remain = (T - seed) % (window - seed)` frames behind them, and a tail window of seed + remain frames when remain exceeds seed (else 0:
    a remainder of at most `seed` frames is dropped).  Pure arithmetic: for T <= seed the callers decide (`window_schedule` raises,
    `streaming.tail_of` answers (0, 0), `inference()` runs no window)."""
    pre, hop = int(seed_frames), int(window) - int(seed_frames)
    rounds, remain = (int(frames) - pre) // hop, (int(frames) - pre) % hop
    return rounds, remain, (pre + remain if remain > pre else 0)


def identity_seed(n, frames=4, dims=SEED_DIMS, device=None):
    """(n, frames, dims) on `device` (None: the host): identity rot6d [1, 0, 0, 0, 1, 0] per joint in the first dims - 7 columns, zero
    trans / foot contact (M:348-351)."""
    seed = torch.zeros(n, frames, dims, device=device)
    seed[:, :, 0:dims - 7:6] = 1.0
    seed[:, :, 4:dims - 7:6] = 1.0
    return seed


class Schedule:
    """What `window_schedule` returns.  rounds / remain / frames: per recording (frames = output frames).  steps: [(start frame, [ids of the
    recordings that run full window i])]; tails: {tail length: [(recording id, start frame)]} in input order."""

    def __init__(self, lengths, rounds, remain, frames, steps, tails, window, seed_frames):
        self.lengths, self.rounds, self.remain, self.frames, self.steps, self.tails = lengths, rounds, remain, frames, steps, tails
        self.window, self.seed_frames = window, seed_frames

    @property
    def n_windows(self):
        """(recording, window) pairs of the schedule, tails included."""
        return sum(len(ids) for _s, ids in self.steps) + sum(len(v) for v in self.tails.values())


def window_schedule(lengths, window=64, seed_frames=4):
    """The windows `EmageAudioModel.inference` (M:364-368, M:380-382, M:428-431) runs for recordings of `lengths` frames, as a lock-step
    schedule -> `Schedule`.  Full windows: `rounds` of them (`split_length`) at starts i * (window - seed), each keeping its first
    window - seed frames.  Tail: seed + remain frames from rounds * (window - seed), kept whole; T < window is a tail only, T == window one
    full window (window - seed frames out, no tail).  Output frames: (window - seed) * rounds + the tail's."""
    pre, hop = int(seed_frames), int(window) - int(seed_frames)
    if hop <= 0:
        raise ValueError(f"window_schedule: window {window} must exceed seed_frames {seed_frames}")
    lengths = [int(t) for t in lengths]
    if any(t <= pre for t in lengths):
        raise ValueError(f"window_schedule: every recording needs more than {pre} frames, got {lengths}")
    splits = [split_length(t, window, pre) for t in lengths]
    rounds, remain = [s[0] for s in splits], [s[1] for s in splits]
    frames = [hop * r + tail for r, _m, tail in splits]
    steps = [(i * hop, [k for k, r in enumerate(rounds) if r > i]) for i in range(max(rounds, default=0))]
    tails = {}
    for k, (r, _m, tail) in enumerate(splits):
        if tail:
            tails.setdefault(tail, []).append((k, r * hop))
    return Schedule(lengths, rounds, remain, frames, steps, tails, int(window), pre)
