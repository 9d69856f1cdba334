"""rep15d on the device: the motion representation the reference's BC / L1div metrics read (emage_utils/motion_rep_transfer.py:51-72).

    rep = motion_rep.motion_rep(poses, joints, pose_fps=30)     # poses (N, 165) or (B, N, 165); joints (N, >= 55, 3) or (B, N, >= 55, 3)
    rep["rep15d"]                                               # (N, 825) or (B, N, 825)

`poses` are the axis-angle poses this package generates (`RecordingRunner`, `LstmRecordingRunner`, `StreamBatch.step()`); `joints` are the
SMPL-X joint positions of the same frames, of which the first 55 are read — the reference takes them from the `smplx` forward with zero
betas, translation, expression, jaw, eyes and global orientation; evaluating the body model is NOT part of this package, so
they come from the caller.  Both may be device tensors or numpy.  One launch (`emage_motion_rep`, csrc/motion_rep.hip): position, velocity
(one-sided differences at the two ends, central ones inside, divided by dt = 1 / pose_fps), rot-6D with the arithmetic of
`ops.axis_angle_to_rot6d`, angular velocity by the same differences.  Every entry of the result is a VIEW of one packed (…, N, 55, 15) fp32
device buffer; pass `out` (that shape, contiguous) to reuse a buffer — the call then allocates nothing when its inputs are fp32 device
tensors, and can be captured in a graph."""
from __future__ import annotations

import numpy as np
import torch

from . import ops

J = ops.REP_JOINTS
POSE_DIMS = 3 * J


def _device_f32(x, device):
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32)))
    return x.to(device=device, dtype=torch.float32)


def motion_rep(poses, joints, pose_fps=30, out=None, device=None):
    """-> dict of position, velocity, angular_velocity (…, N, 55, 3), rotation (…, N, 55, 6), axis_angle (…, N, 165), rep15d (…, N, 825):
    fp32 device tensors, `…` = () for one sequence and (B,) for a batch.  N >= 2 (the differences need two frames, as in the reference)."""
    if poses.ndim not in (2, 3) or poses.shape[-1] != POSE_DIMS or poses.shape[-2] < 2:
        raise ValueError(f"poses: shape {tuple(poses.shape)}, expected (N, {POSE_DIMS}) or (B, N, {POSE_DIMS}) with N >= 2")
    lead, t = tuple(poses.shape[:-2]), int(poses.shape[-2])
    if joints.ndim != poses.ndim + 1 or tuple(joints.shape[:-2]) != lead + (t,) or joints.shape[-2] < J or joints.shape[-1] != 3:
        raise ValueError(f"joints: shape {tuple(joints.shape)}, expected {lead + (t,)} + (>= {J}, 3)")
    if not pose_fps > 0:
        raise ValueError(f"pose_fps {pose_fps}")
    b = lead[0] if lead else 1
    if device is None:
        device = poses.device if torch.is_tensor(poses) else joints.device if torch.is_tensor(joints) else "cuda"
    p = _device_f32(poses, device).reshape(b * t, POSE_DIMS)
    p = p if p.is_contiguous() else p.contiguous()
    jt = _device_f32(joints, device).reshape(b * t, joints.shape[-2], 3)
    if not (jt.stride(2) == 1 and jt.stride(1) == 3 and (b * t == 1 or jt.stride(0) >= POSE_DIMS)):
        jt = jt.contiguous()
    if out is None:
        out = torch.empty(lead + (t, J, 15), dtype=torch.float32, device=p.device)
    elif tuple(out.shape) != lead + (t, J, 15) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"out: expected a contiguous float32 tensor of shape {lead + (t, J, 15)}")
    ops.motion_rep(p, jt, 1.0 / pose_fps, out.view(b, t, J, 15))
    return dict(position=out[..., 0:3], velocity=out[..., 3:6], rotation=out[..., 6:12], axis_angle=p.view(lead + (t, POSE_DIMS)),
                angular_velocity=out[..., 12:15], rep15d=out.view(lead + (t, J * 15)))
