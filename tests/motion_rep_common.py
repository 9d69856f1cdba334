"""Shared pieces of the rep15d tests (test_motion_rep_gpu.py, test_motion_rep_host.py): seeded inputs, a float64 numpy restatement of
emage_utils/motion_rep_transfer.py:51-64 written independently of the kernel, wrong references, and tolerances derived from the operands
in the manner of tests/kernel_checks.py (u = EPS32, never from the kernel's output):
  position          a copy: bit-equal to the input.
  velocity, angular velocity   (a - b) / div with a, b fp32: the subtraction rounds once (u |a - b|), div = float(dt) or 2 float(dt) carries
                    u relative (the doubling is exact), the division rounds once: 3 u |result| to first order; 4 u |result| leaves room
                    for the second-order terms, + the smallest subnormal for results that underflow.
  rot-6D            bit-equal to emage_axis_angle_to_rot6d (tests/test_forward_kernels_gpu.py holds that op to float64); against float64 here:
                    |aa| <= pi + 1: the norm carries 2.5 u relative = <= 11 u absolute on the angle, half of it on the half angle, sin / cos
                    that plus 2 ulp (<= 8 u), the quaternion products and the 2 / |q|^2 scaling six more roundings of values <= 2:
                    <= 64 u per entry."""
import math

import numpy as np
import torch

from kernel_checks import EPS32

J = 55
ROT6D_TOL = 64 * EPS32
WRONG = ("central_at_the_ends", "one_sided_inside", "dt_not_doubled", "across_sequences")


def make_inputs(seed, batch, frames, joints_out=55):
    """poses (batch, frames, 165): rotations up to pi in norm, exact zeros and vectors of norm 1e-9; joints (batch, frames, joints_out, 3): a
    random walk of ~2 cm steps around a ~1 m body, so velocities are ~0.6 m/s.  float32 (what the kernel is given)."""
    rng = np.random.default_rng(seed)
    axis = rng.standard_normal((batch, frames, J, 3))
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    aa = axis * rng.uniform(0, math.pi, size=(batch, frames, J, 1))
    kind = rng.integers(0, 8, size=(batch, frames, J))
    aa[kind == 0] = 0.0
    aa[kind == 1] *= 1e-9 / np.maximum(np.linalg.norm(aa[kind == 1], axis=-1, keepdims=True), 1e-30)
    joints = rng.uniform(-1, 1, size=(batch, 1, joints_out, 3)) + np.cumsum(0.02 * rng.standard_normal((batch, frames, joints_out, 3)), axis=1)
    return aa.reshape(batch, frames, 3 * J).astype(np.float32), joints.astype(np.float32)


def finite_differences(x, dt, wrong=None):
    """motion_rep_transfer.py:53-56 along axis 1 of (B, N, ...)."""
    first, last, mid = (x[:, 1:2] - x[:, 0:1]) / dt, (x[:, -1:] - x[:, -2:-1]) / dt, (x[:, 2:] - x[:, :-2]) / (2 * dt)
    if wrong == "central_at_the_ends":
        first, last = first / 2, last / 2
    if wrong == "one_sided_inside":
        mid = (x[:, 2:] - x[:, 1:-1]) / dt
    if wrong == "dt_not_doubled":
        mid = mid * 2
    return np.concatenate([first, mid, last], axis=1)


def rot6d(aa):
    """rotation_conversions.axis_angle_to_matrix -> matrix_to_rotation_6d in float64: the first two rows of the rotation matrix."""
    angle = np.linalg.norm(aa, axis=-1, keepdims=True)
    d = aa / np.maximum(angle, 1e-300)
    k = np.zeros(aa.shape[:-1] + (3, 3))
    k[..., 0, 1], k[..., 0, 2], k[..., 1, 0], k[..., 1, 2], k[..., 2, 0], k[..., 2, 1] = -d[..., 2], d[..., 1], d[..., 2], -d[..., 0], -d[..., 1], d[..., 0]
    r = np.eye(3) + np.sin(angle)[..., None] * k + (1 - np.cos(angle))[..., None] * (k @ k)
    return r[..., :2, :].reshape(aa.shape[:-1] + (6,))


def reference(poses, joints, pose_fps=30, wrong=None):
    """(B, N, 165), (B, N, >= 55, 3) -> dict of float64 arrays shaped like motion_rep.motion_rep's, batch kept."""
    p, j = np.asarray(poses, dtype=np.float64), np.asarray(joints, dtype=np.float64)[:, :, :J]
    b, n = p.shape[:2]
    dt = 1.0 / pose_fps
    if wrong == "across_sequences":                      # the batch treated as one long sequence: differences cross the sequence ends
        vel = finite_differences(j.reshape(1, b * n, J, 3), dt).reshape(b, n, J, 3)
        ang = finite_differences(p.reshape(1, b * n, -1), dt).reshape(b, n, J, 3)
    else:
        vel, ang = finite_differences(j, dt, wrong), finite_differences(p, dt, wrong).reshape(b, n, J, 3)
    out = dict(position=j, velocity=vel, rotation=rot6d(p.reshape(b, n, J, 3)), angular_velocity=ang)
    out["rep15d"] = np.concatenate([out["position"], out["velocity"], out["rotation"], out["angular_velocity"]], axis=3).reshape(b, n, J * 15)
    return out


def difference_tolerance(ref):
    return 4 * EPS32 * np.abs(ref) + 2.0 ** -149


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))
