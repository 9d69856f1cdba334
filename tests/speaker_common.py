"""Shared pieces of the per-clip speaker-id tests: the multi-speaker golden (tests/golden/train_step_speakers.npz, the REAL reference step
with speaker_dims = 4 and ids [2, 0, 2, 1]), the oracle step restated with ids (tools/workloads.py) run once, product models with more than
one speaker row, and small clip stores whose recordings belong to different speakers."""
import os

import numpy as np
import torch

import common
from pantomatrix_amd import data, synthetic
from pantomatrix_amd.configuration_emage_audio import EmageAudioConfig

GOLDEN = "train_step_speakers.npz"
TABLES = ("speaker_embedding_body.weight", "speaker_embedding_face.weight")
LOSS_KEYS = ("rec_seed", "cls_seed", "rec_audio", "cls_audio", "rec_mask", "cls_mask", "all")

_CACHE = {}


def golden(golden_dir):
    return np.load(os.path.join(golden_dir, GOLDEN))


def audio_cfg(speaker_dims):
    return dict(common.cfg_dicts()[0], speaker_dims=int(speaker_dims))


def oracle_step(g, backward=False):
    """The recorded oracle step on the golden's batch and ids — once per process and flavour; callers must not modify the tensors."""
    key = ("step", bool(backward))
    if key not in _CACHE:
        from tools import workloads
        _CACHE[key] = workloads.oracle_train_step_recorded(int(g["seed"]), int(g["iteration"]), bs=int(g["bs"]), backward=backward,
                                                           speaker_id=[int(i) for i in g["speaker_ids"]], speaker_dims=int(g["speaker_dims"]))
    return _CACHE[key]


def product_models(speaker_dims, precision="fp32", device="cpu", seed=0):
    """common.product_models with `speaker_dims` rows in the two speaker tables (the VQ models are the usual ones)."""
    import pantomatrix_amd as pa
    cfg = pa.EmageAudioConfig(**audio_cfg(speaker_dims))
    key = ("state", int(speaker_dims), seed)
    if key not in _CACHE:
        _CACHE[key] = synthetic.audio_model_state(cfg, seed)
    model = pa.EmageAudioModel(cfg)
    model.load_state_dict(_CACHE[key])
    model.set_precision(precision)
    _, vq = common.product_models(seed=seed, precision=precision, device=device)
    if device != "cpu":
        model.to(device)
    return model.eval(), vq


def oracle_audio_model(speaker_dims, seed=0):
    from oracle import emage_oracle as orc
    cfg = EmageAudioConfig(**audio_cfg(speaker_dims))
    return orc.AudioModel(synthetic.audio_model_state(cfg, seed), cfg)


# ---- a small store: 3 recordings of speakers [2, 0, 2], 7 clips of 8 frames ---------------------------------------------------------
STORE_SPEAKERS = (2, 0, 2)
STORE_FRAMES, STORE_CLIP = (20, 12, 17), 8
STORE_CLIPS = ((0, 0, 8), (0, 5, 13), (0, 12, 20), (1, 0, 8), (1, 4, 12), (2, 1, 9), (2, 9, 17))


def speaker_store(device, speakers=STORE_SPEAKERS, audio_sr=16000):
    g = np.random.default_rng(3)
    spf = data.samples_per_frame(audio_sr)
    recs = []
    for f, s in zip(STORE_FRAMES, speakers):
        rec = dict(poses=g.standard_normal((f, 165)).astype(np.float32), expressions=g.standard_normal((f, 100)).astype(np.float32),
                   trans=g.standard_normal((f, 3)).astype(np.float32), foot_contact=(g.random((f, 4)) > 0.5).astype(np.float32),
                   audio=g.integers(-3000, 3000, f * spf).astype(np.int16))
        if s is not None:
            rec["speaker"] = s
        recs.append(rec)
    return data.ClipStore.from_arrays(recs, list(STORE_CLIPS), device, audio_sr=audio_sr)

