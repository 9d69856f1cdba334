"""Generate tests/golden/reference_{inference_rec,inference_cls,decode,formats,lstm}.npz from the REAL reference (build container only):
    python tests/golden/make_golden_reference.py
What the reference computes on the seeded inputs of tests/test_oracle_vs_reference.py, tests/test_formats.py::
test_formats_match_reference and tests/test_lstm_models_oracle.py::test_matches_reference_live, so those tests run anywhere.
The EMAGE outputs are stored as integer multiples of a power-of-two step (`*_step`; the inference outputs as frame-to-frame
differences of those multiples, which compress better); the tests tighten their tolerance by half a step, so a quantised value
passing the test means the exact one passes the original tolerance.  A step leaves room for that: it is below the tolerance
less the oracle's error (measured: 6e-6 of 2e-4 for inference, 0 of 1e-4 for decode).  The DisCo / CaMN motion is
already in lstm_models.npz (tests/golden/make_golden_lstm.py, same weights and inputs): only the other outputs go here."""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import common  # noqa: E402
import test_formats  # noqa: E402
import test_lstm_models_oracle as tlo  # noqa: E402
import test_oracle_vs_reference as tovr  # noqa: E402
from oracle import emage_oracle as orc  # noqa: E402
from oracle import reference_harness as rh  # noqa: E402


INFER_STEP, DECODE_STEP = 2.0 ** -13, 2.0 ** -14        # the tests' tolerances: 2e-4 / 1e-4


def quantised(a, step, frame_deltas=False):
    """int32 multiples of `step`; with frame_deltas, their differences along axis 1 (np.cumsum(..., axis=1) restores them)."""
    q = np.round(np.asarray(a, np.float64) / step)
    if frame_deltas:
        q = np.diff(q, axis=1, prepend=0)
    return q.astype(np.int32)


def key_table(sd):
    """A state dict's keys in order and their shapes (comma-joined dims)."""
    return np.array(list(sd.keys())), np.array([",".join(str(d) for d in v.shape) for v in sd.values()])


def inference(rec, cls):
    """The latents (rec_*) and the code logits (cls_*) of one 133-frame clip, one file each; the state-dict key table with the latents."""
    acfg, vqc, gc = common.cfg_dicts()
    model, vq = rh.build_reference(acfg, vqc, gc, seed=0)
    rec["audio_keys"], rec["audio_shapes"] = key_table(model.state_dict())
    audio, spk = tovr.inference_inputs()
    with torch.no_grad():
        r = model.inference(audio, spk, vq)
    for out in (rec, cls):
        out["infer_step"] = INFER_STEP
    for k in orc.OUT_KEYS:
        (rec if k.startswith("rec_") else cls)[f"infer_{k}"] = quantised(r[k].numpy(), INFER_STEP, frame_deltas=True)


def decode(out):
    acfg, vqc, gc = common.cfg_dicts()
    _, vq = rh.build_reference(acfg, vqc, gc, seed=0)
    idx, lat = tovr.decode_inputs()
    with torch.no_grad():
        r = vq.decode(face_latent=lat, upper_index=idx["upper"], hands_index=idx["hands"], lower_index=idx["lower"],
                      get_global_motion=True, ref_trans=torch.zeros(1, 3))
    out["decode_step"] = DECODE_STEP
    for k in tovr.DECODE_KEYS:
        out[f"decode_{k}"] = quantised(r[k].numpy(), DECODE_STEP)


def formats(out):
    sys.modules.setdefault("smplx", types.ModuleType("smplx"))
    sys.path.insert(0, rh.REFERENCE_ROOT)
    try:
        from emage_utils import motion_io as ref
    finally:
        sys.path.remove(rh.REFERENCE_ROOT)
    x, e, t = test_formats.reference_inputs()
    for name in test_formats.MASKS:
        out[f"fmt_mask_{name}"] = np.array(ref.MASK_DICT[name], dtype=bool)
        s = ref.select_with_mask(x, ref.MASK_DICT[name])
        out[f"fmt_select_{name}"] = s
        out[f"fmt_recover_{name}"] = ref.recover_from_mask(s, ref.MASK_DICT[name])
    out["fmt_upsample3"] = ref.time_upsample_numpy(x, 3)
    with tempfile.TemporaryDirectory() as tmp:
        ref.beat_format_save(os.path.join(tmp, "b.npz"), x, expressions=e, trans=t, upsample=2)
        b = np.load(os.path.join(tmp, "b.npz"), allow_pickle=True)
        out["fmt_save_files"] = np.array(sorted(b.files))
        for k in test_formats.SAVED_ARRAYS:
            out[f"fmt_save_{k}"] = b[k]


def lstm(out):
    motion_golden = np.load(os.path.join(HERE, "lstm_models.npz"))
    for kind in ("disco", "camn"):
        sd = tlo.weights(kind)
        model = rh.build_reference_lstm_model(kind, tlo.CFG, sd)      # strict load: the spec IS the reference's key / shape set
        out[f"lstm_{kind}_keys"], out[f"lstm_{kind}_shapes"] = key_table(model.state_dict())
        for wsm in (False, True):
            tag = tlo.case_tag(wsm)
            audio, spk, motion = tlo.inputs(with_seed_motion=wsm)
            with torch.no_grad():
                ref = model(audio, spk, seed_frames=tlo.CFG["seed_frames"], seed_motion=motion)
            out[f"lstm_{kind}_outputs"] = np.array(list(ref.keys()))
            out[f"lstm_{kind}_motion_shape"] = np.array(ref["motion"].shape)
            assert np.array_equal(ref["motion"].reshape(2, -1, 258).numpy(), motion_golden[f"{kind}_{tag}_motion"])
            assert np.array_equal(ref["motion_axis_angle"].numpy(), motion_golden[f"{kind}_{tag}_axis_angle"])
            for k, v in ref.items():
                if k in ("motion", "motion_axis_angle"):
                    continue
                if f"lstm_{kind}_{k}" in out:         # the audio features do not depend on the seed motion: stored once
                    assert np.array_equal(out[f"lstm_{kind}_{k}"], v.numpy()), k
                out[f"lstm_{kind}_{k}"] = v.numpy()


def main():
    assert rh.available(), "needs the reference tree"
    files = {name: {} for name in ("inference_rec", "inference_cls", "decode", "formats", "lstm")}
    inference(files["inference_rec"], files["inference_cls"])
    decode(files["decode"])
    formats(files["formats"])
    lstm(files["lstm"])
    for name, out in files.items():
        path = os.path.join(HERE, f"reference_{name}.npz")
        np.savez_compressed(path, **out)
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
