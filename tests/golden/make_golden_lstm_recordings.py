"""Generate tests/golden/lstm_recordings.npz from the REAL reference DisCo / CaMN modules (build container only): each of the three
recordings of tests/test_lstm_ragged_host.py alone at B = 1, as the reference's test_disco_audio.py / test_camn_audio.py run a file.
    python tests/golden/make_golden_lstm_recordings.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import lstm_models_oracle as lo  # noqa: E402
from oracle import reference_harness as rh  # noqa: E402
from test_lstm_models_oracle import CFG, weights  # noqa: E402
from test_lstm_ragged_host import OWN_ERROR_SHARE, ragged_inputs  # noqa: E402


def own_error(audios, spk):
    """The largest |float32 - float64| of the oracle's axis-angle output over both models and all recordings: how much of the 1e-3
    axis-angle bar the reference's own arithmetic uses up on these waveforms (see RAGGED_SEED)."""
    worst = 0.0
    for kind in ("disco", "camn"):
        sd = weights(kind)
        sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
        fn = lo.disco_forward if kind == "disco" else lo.camn_forward
        for r, audio in enumerate(audios):
            with torch.no_grad():
                o32 = fn(sd, CFG, audio[None], spk[r].view(1, 1), CFG["seed_frames"], None)
                o64 = fn(sd64, CFG, audio[None].double(), spk[r].view(1, 1), CFG["seed_frames"], None)
            worst = max(worst, float((o32["motion_axis_angle"].double() - o64["motion_axis_angle"]).abs().max()))
    return worst


def main():
    assert rh.available(), "needs the reference checkout"
    audios, spk = ragged_inputs()
    err = own_error(audios, spk)
    print(f"own float32 error of the oracle's axis-angle output on these waveforms: {err:.2e}")
    assert err <= OWN_ERROR_SHARE * 1e-3, "choose another RAGGED_SEED: the reference's own rounding uses up the axis-angle bar here"
    out = {}
    for kind in ("disco", "camn"):
        model = rh.build_reference_lstm_model(kind, CFG, weights(kind))
        for r, audio in enumerate(audios):
            with torch.no_grad():
                ref = model(audio[None], spk[r].view(1, 1), seed_frames=CFG["seed_frames"], seed_motion=None)
            t = ref["motion_axis_angle"].shape[1]
            out[f"{kind}_{r}_motion"] = ref["motion"].reshape(t, -1).numpy()
            out[f"{kind}_{r}_axis_angle"] = ref["motion_axis_angle"].reshape(t, 165).numpy()
    path = os.path.join(HERE, "lstm_recordings.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
