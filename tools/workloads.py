"""Seeded synthetic workloads — model builders shared by `bench.py`, `__graft_entry__.smoke()`, the scripts in tools/ and the tests
(tests/common.py re-exports them): the configurations of SURVEY.md §8(d), synthetic weights from `pantomatrix_amd.synthetic`, the
product classes loaded with them, and — for the CHECKER side only (bench.py's `cpu_baseline` / error prints, smoke(), tests) — the CPU
oracle objects built from the same weights.  The oracle imports are local to the functions that need them: building a product model
never touches `oracle/`."""
from __future__ import annotations

import functools
import json

import torch

from pantomatrix_amd import spec, synthetic
from pantomatrix_amd.configuration_emage_audio import EmageAudioConfig, EmageVQVAEConvConfig, EmageVAEConvConfig

PARTS = ("face", "upper", "hands", "lower")
LSTM_CFG = dict(spec.LSTM_MODEL_DEFAULTS)          # configs/disco_audio.yaml, configs/camn_audio.yaml


def cfg_dicts(vae_layer=2, global_layer=4, global_length=240):
    return (dict(spec.EMAGE_AUDIO_DEFAULTS), {p: spec.default_vq_cfg_dict(p, vae_layer) for p in PARTS},
            spec.default_global_cfg_dict(global_layer, global_length))


_STATE_CACHE = {}


def _synthetic_state(make, *key):
    """The seeded synthetic weights of a model, generated once per process (`load_state_dict` copies them into the parameters, so the
    cached tensors are never aliased by a model; the suites build ~100 model sets from the same seeds)."""
    if key not in _STATE_CACHE:
        _STATE_CACHE[key] = make()
    return _STATE_CACHE[key]


def product_models(seed=0, vae_layer=2, precision="fp32", device="cpu"):
    """pantomatrix_amd model objects (EmageAudioModel, EmageVQModel) loaded with the seeded synthetic weights."""
    import pantomatrix_amd as pa
    acfg, vqc, gc = cfg_dicts(vae_layer)
    cfg = pa.EmageAudioConfig(**acfg)
    model = pa.EmageAudioModel(cfg)
    model.load_state_dict(_synthetic_state(lambda: synthetic.audio_model_state(cfg, seed), "audio", json.dumps(acfg, sort_keys=True), seed))
    parts = {}
    for p in PARTS:
        c = pa.EmageVQVAEConvConfig(**vqc[p])
        parts[p] = pa.EmageVQVAEConv(c)
        parts[p].load_state_dict(_synthetic_state(lambda: synthetic.vqvae_state(c, p, seed), "vq", p, json.dumps(vqc[p], sort_keys=True), seed))
    g = pa.EmageVAEConv(pa.EmageVAEConvConfig(**gc))
    g.load_state_dict(_synthetic_state(lambda: synthetic.vae_state(pa.EmageVAEConvConfig(**gc), seed), "global", json.dumps(gc, sort_keys=True), seed))
    vq = pa.EmageVQModel(face_model=parts["face"], upper_model=parts["upper"], hands_model=parts["hands"],
                         lower_model=parts["lower"], global_model=g)
    model.set_precision(precision)
    vq.set_precision(precision)
    if device != "cpu":
        model.to(device)
        vq.to(device)
    return model.eval(), vq.eval()


def product_infer_clip(model, vq, audio, speaker_id=None):
    """test_emage_audio.py:16-53 against the product classes; returns numpy (poses, expressions, trans)."""
    bs = audio.shape[0]
    dev = model.device
    if speaker_id is None:
        speaker_id = torch.zeros(bs, 1, dtype=torch.long, device=dev)
    lat = model.inference(audio.to(dev), speaker_id, vq)
    pred = vq.decode(**model._select_codes(lat), get_global_motion=True, ref_trans=torch.zeros(1, 3, device=dev))
    return (pred["motion_axis_angle"].cpu().numpy(), pred["expression"].cpu().numpy(), pred["trans"].cpu().numpy()), lat


def train_batch(bs=2, t=64, seed=5):
    """One training batch in the shapes `BEAT2DatasetEamgeFootContact.__getitem__` returns (datasets/beat2.py:97-129)."""
    g = torch.Generator().manual_seed(seed)
    return dict(motion=0.3 * torch.randn(bs, t, 165, generator=g), audio=0.1 * torch.randn(bs, t * 16000 // 30, generator=g),
                expressions=0.5 * torch.randn(bs, t, 100, generator=g), trans=0.1 * torch.randn(bs, t, 3, generator=g),
                foot_contact=(torch.rand(bs, t, 4, generator=g) > 0.5).float())


# ---- DisCo / CaMN -------------------------------------------------------------------------------------------------------------------
def lstm_weights(kind, seed=0):
    """Seeded synthetic state dict of DiscoAudioModel / CamnAudioModel (kind "disco" / "camn")."""
    from pantomatrix_amd import modeling_lstm_audio as L
    ccls = L.DiscoAudioConfig if kind == "disco" else L.CamnAudioConfig
    cfg = ccls(**LSTM_CFG)
    sp = spec.disco_model_spec(cfg) if kind == "disco" else spec.camn_model_spec(cfg)
    return _synthetic_state(lambda: synthetic.state_dict_from_spec(sp, seed, None, prefix=f"{kind}_audio/"), "lstm", kind, seed)


def lstm_product(kind, precision="f16x3", device=None):
    from pantomatrix_amd import modeling_lstm_audio as L
    cls, ccls = (L.DiscoAudioModel, L.DiscoAudioConfig) if kind == "disco" else (L.CamnAudioModel, L.CamnAudioConfig)
    m = cls(ccls(**LSTM_CFG)).set_precision(precision)
    m.load_state_dict(lstm_weights(kind))
    return m.to(device) if device else m


# ---- the checker side (CPU oracle; bench.py's cpu_baseline leg, smoke(), tests) ---------------------------------------------------------
@functools.lru_cache(maxsize=4)
def oracle_models(seed=0, vae_layer=2):
    from oracle import emage_oracle as orc
    acfg, vqc, gc = cfg_dicts(vae_layer)
    cfg = EmageAudioConfig(**acfg)
    model = orc.AudioModel(synthetic.audio_model_state(cfg, seed), cfg)
    parts = [orc.VQVAE(synthetic.vqvae_state(EmageVQVAEConvConfig(**vqc[p]), p, seed), EmageVQVAEConvConfig(**vqc[p])) for p in PARTS]
    vq = orc.VQModel(*parts, orc.VAE(synthetic.vae_state(EmageVAEConvConfig(**gc), seed), EmageVAEConvConfig(**gc)))
    return model, vq


def lstm_oracle(kind, sd, audio, spk, motion=None):
    from oracle import lstm_models_oracle as lo
    fn = lo.disco_forward if kind == "disco" else lo.camn_forward
    with torch.no_grad():
        return fn(sd, LSTM_CFG, audio, spk, LSTM_CFG["seed_frames"], motion)


def _train_step_losses_with_ids(tro, speaker_id):
    """oracle.emage_train_oracle.train_step_losses restated with the given per-clip speaker ids in place of its zeros: the same calls in
    the same order (forward 1, `torch.rand` for the random mask, forward 2, forward 3), so the generator draws are the oracle's."""
    def train_step_losses(sd, vq, cfg, batch, iteration, p=tro.DROPOUT_P):
        index, latent, masked_motion = tro.targets(vq, batch["motion"], batch["expressions"], batch["trans"], batch["foot_contact"])
        bs, t = masked_motion.shape[:2]
        spk = torch.as_tensor(speaker_id, dtype=torch.long).reshape(bs, 1)
        stats, loss = {}, {}
        mask = torch.ones_like(masked_motion)
        mask[:, :cfg.seed_frames] = 0
        pred = tro.forward_train(sd, batch["audio"], spk, masked_motion, mask, True, p, stats)
        loss["rec_seed"], loss["cls_seed"] = tro.rec_loss(pred, latent, cfg), tro.cls_loss(pred, index, cfg)
        mask_ratio = (iteration / 135 * 400) * 0.95 + 0.05
        mask = (torch.rand(bs, t, cfg.pose_dims + 3 + 4) < mask_ratio).float()
        pred = tro.forward_train(sd, batch["audio"], spk, masked_motion, mask, True, p, stats)
        loss["rec_audio"], loss["cls_audio"] = tro.rec_loss(pred, latent, cfg), tro.cls_loss(pred, index, cfg)
        pred = tro.forward_train(sd, batch["audio"], spk, masked_motion, mask, False, p, stats)
        loss["rec_mask"], loss["cls_mask"] = tro.rec_loss(pred, latent, cfg), tro.cls_loss(pred, index, cfg)
        loss["all"] = sum(loss.values())
        return loss, stats
    return train_step_losses


def oracle_train_step_recorded(seed, iteration, bs=2, backward=False, batch=None, speaker_id=None, speaker_dims=None):
    """One training step of the CPU oracle (oracle/emage_train_oracle.py: the reference's train_val_fn restated) with what a device run
    needs to REPEAT it recorded: every forward's dropout masks (the oracle issues the reference's generator draws; a recorded mask is
    exactly the tensor torch multiplies with — the oracle's result is unchanged bit for bit) and the random motion mask of forwards 2 / 3.
    backward=False: the three forwards and their losses (`train_step_losses`); True: the whole step (`train_step`: + gradients, Adam).
    speaker_id: one speaker-table row per clip (the oracle's own step hard-codes zeros, so its lines are restated with the ids:
    `_train_step_losses_with_ids`); None = the oracle's step itself.  speaker_dims: rows of the two speaker tables (None: the default
    configuration's).
    -> dict(batch, losses {name: float}, masks [forward 1, 2, 3], random_mask, stats (BatchNorm buffers), grads, new_sd)."""
    import contextlib
    import torch.nn.functional as F
    from oracle import emage_train_oracle as tro
    cfg = EmageAudioConfig(**(cfg_dicts()[0] if speaker_dims is None else dict(cfg_dicts()[0], speaker_dims=int(speaker_dims))))
    _, vq = oracle_models()
    sd = synthetic.audio_model_state(cfg, 0)
    batch = train_batch(bs=bs) if batch is None else batch
    per_forward, motion_masks = [], []

    @contextlib.contextmanager
    def recorded(store):
        saved = tro._drop

        def _drop(x, p):
            if p <= 0:
                return x
            m = F.dropout(torch.ones_like(x), p, training=True)       # ones_like keeps x's memory format: the same draws in the same order
            store.append(m.detach())
            return x * m

        tro._drop = _drop
        try:
            yield store
        finally:
            tro._drop = saved

    orig = tro.forward_train

    def spy(sd_, audio, spk, motion, mask, use_audio=True, p=tro.DROPOUT_P, new_stats=None):
        masks = []
        with recorded(masks):
            out = orig(sd_, audio, spk, motion, mask, use_audio=use_audio, p=p, new_stats=new_stats)
        per_forward.append(masks)
        motion_masks.append(mask.clone())
        return out

    tro.forward_train = spy
    orig_losses = tro.train_step_losses
    if speaker_id is not None:
        tro.train_step_losses = _train_step_losses_with_ids(tro, speaker_id)
    grads, new_sd = None, None
    try:
        if backward:
            losses, grads, new_sd, _ = tro.train_step(sd, vq, cfg, batch, iteration, seed=seed)
            stats = {k: v for k, v in new_sd.items() if k.endswith((".running_mean", ".running_var", ".num_batches_tracked"))}
        else:
            torch.manual_seed(seed)
            with torch.no_grad():
                losses, stats = tro.train_step_losses(sd, vq, cfg, batch, iteration)
    finally:
        tro.forward_train, tro.train_step_losses = orig, orig_losses
    return dict(batch=batch, losses={k: float(v) for k, v in losses.items()}, masks=per_forward, random_mask=motion_masks[1], stats=stats,
                grads=grads, new_sd=new_sd, recorder=recorded)
