"""rep15d without a GPU (pantomatrix_amd/motion_rep.py): the float64 reference's own properties, the module on the fp32 stand-in of
tests/fake_motion_rep_ops.py (shapes, views, numpy and tensor inputs, the `out` buffer, argument errors), and the argument validation of
the new entry point."""
import numpy as np
import pytest
import torch

import fake_motion_rep_ops
import fake_ops
import motion_rep_common as mc
from kernel_checks import _cmp, _far
from pantomatrix_amd import _lib, motion_rep as MR


def test_reference_differences_are_exact_on_linear_motion_and_wrong_references_differ():
    n, dt = 7, 1.0 / 30
    line = (np.arange(n, dtype=np.float64)[None, :, None] * np.array([0.5, -1.0, 2.0])).repeat(2, axis=0)       # x[n] = n * slope
    assert np.allclose(mc.finite_differences(line, dt), np.array([0.5, -1.0, 2.0]) / dt, rtol=1e-14, atol=0)
    poses, joints = mc.make_inputs(1, 3, 9)
    ref = mc.reference(poses, joints)
    assert ref["rep15d"].shape == (3, 9, 825) and np.array_equal(ref["rep15d"].reshape(3, 9, 55, 15)[..., 3:6], ref["velocity"])
    for wrong in mc.WRONG:
        bad = mc.reference(poses, joints, wrong=wrong)
        for k in ("velocity", "angular_velocity"):
            _far(f"{wrong} {k}", mc.t(ref[k]), mc.t(bad[k]), mc.t(mc.difference_tolerance(ref[k])))
    # the rot-6D block is the first two rows of a rotation matrix: unit, orthogonal
    r = ref["rotation"].reshape(-1, 2, 3)
    assert np.abs(np.einsum("nij,nkj->nik", r, r) - np.eye(2)).max() < 1e-12


@pytest.mark.parametrize("batch,frames", [(None, 2), (None, 9), (3, 5)])
def test_module_on_the_stand_in(batch, frames):
    poses, joints = mc.make_inputs(2, batch or 1, frames, joints_out=60)                # 60 joints given, 55 read
    ref = mc.reference(poses, joints)
    p, j = (poses, joints) if batch else (poses[0], joints[0])
    lead = (batch,) if batch else ()
    with fake_motion_rep_ops.installed():
        rep = MR.motion_rep(p, j, device="cpu")                                        # numpy in
        again = MR.motion_rep(torch.from_numpy(p), torch.from_numpy(j), out=torch.empty(lead + (frames, 55, 15)))
        assert fake_ops.CALLS.count("motion_rep") == 2
    assert rep["rep15d"].shape == lead + (frames, 825) and rep["position"].shape == lead + (frames, 55, 3)
    assert rep["rotation"].shape == lead + (frames, 55, 6) and rep["axis_angle"].shape == lead + (frames, 165)
    for k in rep:
        assert torch.equal(rep[k], again[k]) and rep[k].dtype == torch.float32, k
    r15 = rep["rep15d"].reshape(lead + (frames, 55, 15))
    for k, sl in (("position", slice(0, 3)), ("velocity", slice(3, 6)), ("rotation", slice(6, 12)), ("angular_velocity", slice(12, 15))):
        assert rep[k].data_ptr() == r15[..., sl].data_ptr() and torch.equal(rep[k], r15[..., sl]), f"{k} is a view of the packed buffer"
    assert torch.equal(rep["position"].reshape(-1, 55, 3), torch.from_numpy(joints.reshape(-1, 60, 3)[:, :55]))
    for k in ("velocity", "angular_velocity"):
        _cmp(k, rep[k].reshape(batch or 1, frames, 55, 3), mc.t(ref[k]), mc.t(mc.difference_tolerance(ref[k])))
    _cmp("rotation", rep["rotation"].reshape(batch or 1, frames, 55, 6), mc.t(ref["rotation"]), mc.ROT6D_TOL)


def test_module_rejects_bad_arguments():
    poses, joints = mc.make_inputs(3, 1, 4)
    with fake_motion_rep_ops.installed():
        for p, j, kw in ((poses[0, :1], joints[0, :1], {}),                               # one frame: no difference to take
                         (poses[0, :, :164], joints[0], {}), (poses[0], joints[0, :, :54], {}), (poses[0], joints[0, :3], {}),
                         (poses, joints[0], {}), (poses[0], joints[0], dict(pose_fps=0)),
                         (poses[0], joints[0], dict(out=torch.empty(4, 55, 14)))):
            with pytest.raises(ValueError):
                MR.motion_rep(p, j, device="cpu", **kw)


def test_entry_point_validates_without_a_gpu():
    """Invalid arguments are rejected before any launch (EMAGE_EINVAL = -1), as tests/test_abi.py checks for the older entry points."""
    lib = _lib.load()
    p = 4096                                                                           # a non-NULL pointer value: nothing is dereferenced
    dt = 1.0 / 30
    assert lib.emage_motion_rep(None, p, 165, dt, p, 1, 5, None) == -1 and lib.emage_motion_rep(p, None, 165, dt, p, 1, 5, None) == -1
    assert lib.emage_motion_rep(p, p, 165, dt, None, 1, 5, None) == -1
    assert lib.emage_motion_rep(p, p, 165, dt, p, 1, 1, None) == -1 and lib.emage_motion_rep(p, p, 165, dt, p, 0, 5, None) == -1
    assert lib.emage_motion_rep(p, p, 164, dt, p, 1, 5, None) == -1 and lib.emage_motion_rep(p, p, 165, 0.0, p, 1, 5, None) == -1
    assert lib.emage_motion_rep(p, p, 165, float("nan"), p, 1, 5, None) == -1
    assert lib.emage_motion_rep(p, p, 165, dt, p, 2 ** 31 - 1, 2 ** 31 - 1, None) == -1  # beyond the grid limit
