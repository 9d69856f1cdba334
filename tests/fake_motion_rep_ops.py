"""TEST-ONLY CPU stand-in of emage_motion_rep (include/emage_hip.h), restated in fp32 torch from the header's text in the manner of
tests/fake_stream_ops.py: `installed()` is `fake_ops.installed()` plus `ops.motion_rep` on host tensors, so `motion_rep.motion_rep` runs
without a GPU.  Calls are recorded in `fake_ops.CALLS` as "motion_rep"."""
import contextlib

import numpy as np
import torch

import fake_ops
from pantomatrix_amd import ops

J = 55


def motion_rep(poses, joints, dt, rep):
    fake_ops.CALLS.append("motion_rep")
    b, t = rep.shape[0], rep.shape[1]
    assert t >= 2 and poses.shape == (b * t, 3 * J) and joints.shape[0] == b * t and joints.shape[1] >= J
    dt = np.float32(dt)

    def diff(x):                                         # fp32 subtraction, then an fp32 division by float(dt) or 2 float(dt)
        return torch.cat([(x[:, 1:2] - x[:, 0:1]) / dt, (x[:, 2:] - x[:, :-2]) / (np.float32(2) * dt), (x[:, -1:] - x[:, -2:-1]) / dt], dim=1)
    pos = joints[:, :J].reshape(b, t, J, 3)
    aa = poses.view(b, t, J, 3)
    rep[..., 0:3], rep[..., 3:6] = pos, diff(pos)
    rep[..., 6:12] = ops.axis_angle_to_rot6d(aa.reshape(-1, 3)).view(b, t, J, 6)
    rep[..., 12:15] = diff(aa)


@contextlib.contextmanager
def installed():
    with fake_ops.installed():
        saved = ops.motion_rep
        try:
            ops.motion_rep = motion_rep
            yield
        finally:
            ops.motion_rep = saved
