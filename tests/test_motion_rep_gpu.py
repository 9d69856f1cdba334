"""rep15d on the MI355X (csrc/motion_rep.hip, pantomatrix_amd/motion_rep.py) against the float64 restatement of tests/motion_rep_common.py:
sequences of 2 frames (only the one-sided ends), 3 (one central difference) and 40, one sequence and a batch of 3 (no difference may cross
a sequence end), 300 frames x 5 (more than one block per sequence), joints rows of a wider pitch, a NaN-filled output buffer, the rot-6D
block bit-equal to `ops.axis_angle_to_rot6d`, a capture.  Tolerances are derived there; every comparison prints its margin."""
import numpy as np
import pytest
import torch

import motion_rep_common as mc
from kernel_checks import _cmp, _far, _nan_outside, _nans
from pantomatrix_amd import motion_rep as MR, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"


def check(rep, poses, joints, batch, frames, label, wrongs=()):
    ref = mc.reference(poses, joints)
    shaped = lambda k, w: rep[k].reshape(batch, frames, 55, w)
    assert torch.equal(shaped("position", 3).cpu(), torch.from_numpy(joints[:, :, :55])), "positions are copied"
    rot = ops.axis_angle_to_rot6d(torch.from_numpy(poses).to(DEV).reshape(-1, 3))
    assert torch.equal(rep["rotation"].reshape(-1, 6), rot), "the rot-6D block is emage_axis_angle_to_rot6d's bits"
    _cmp(label + " rotation", shaped("rotation", 6), mc.t(ref["rotation"]), mc.ROT6D_TOL)
    for k in ("velocity", "angular_velocity"):
        tol = mc.t(mc.difference_tolerance(ref[k]))
        _cmp(f"{label} {k}", shaped(k, 3), mc.t(ref[k]), tol)
        for wrong in wrongs:
            _far(f"{label} {wrong} {k}", shaped(k, 3), mc.t(mc.reference(poses, joints, wrong=wrong)[k]), tol)
    _cmp(label + " rep15d", rep["rep15d"].reshape(batch, frames, 825), mc.t(ref["rep15d"]),
         mc.t(np.maximum(mc.difference_tolerance(ref["rep15d"]), mc.ROT6D_TOL)))


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("frames", [2, 3, 40])
def test_motion_rep_matches_float64(frames, batch):
    poses, joints = mc.make_inputs(10 * frames + batch, batch, frames)
    p, j = (poses, joints) if batch > 1 else (poses[0], joints[0])
    rep = MR.motion_rep(torch.from_numpy(p).to(DEV), torch.from_numpy(j).to(DEV))
    lead = (batch,) if batch > 1 else ()
    assert rep["rep15d"].shape == lead + (frames, 825) and rep["rep15d"].is_cuda and rep["velocity"].shape == lead + (frames, 55, 3)
    wrongs = [w for w in mc.WRONG if (w != "across_sequences" or batch > 1) and (w in ("central_at_the_ends", "across_sequences") or frames > 2)]
    check(rep, poses, joints, batch, frames, f"N={frames} B={batch}", wrongs)
    again = MR.motion_rep(p, j)                                                        # numpy in: the same bits
    assert all(torch.equal(rep[k], again[k]) for k in rep)


def test_many_blocks_a_wider_joint_pitch_and_an_untouched_buffer():
    batch, frames = 5, 300                                                             # 82 500 threads: 323 blocks, sequences end inside blocks
    poses, joints = mc.make_inputs(7, batch, frames, joints_out=67)                    # 67 joints per frame given (pitch 201), 55 read
    buf = _nans(batch + 1, frames, 55, 15)
    wide = _nans(batch * frames, 70, 3)                                                # the joints as rows of a still wider buffer (pitch 210)
    wide[:, :67] = torch.from_numpy(joints).to(DEV).reshape(-1, 67, 3)
    ops.motion_rep(torch.from_numpy(poses).to(DEV).reshape(-1, 165), wide[:, :67], 1.0 / 30, buf[:batch])
    _nan_outside("rep", buf, slice(0, batch))
    rep = MR.motion_rep(torch.from_numpy(poses).to(DEV), torch.from_numpy(joints).to(DEV))
    assert torch.equal(rep["rep15d"].reshape(batch, frames, 55, 15), buf[:batch])
    check(rep, poses, joints, batch, frames, "N=300 B=5", mc.WRONG)
    assert bool(torch.isnan(wide[:, 67:]).all())


def test_other_frame_rates_and_a_capture():
    poses, joints = mc.make_inputs(8, 2, 40)
    p, j = torch.from_numpy(poses).to(DEV), torch.from_numpy(joints).to(DEV)
    rep15 = MR.motion_rep(p, j, pose_fps=15)
    ref15 = mc.reference(poses, joints, pose_fps=15)
    _cmp("15 fps velocity", rep15["velocity"], mc.t(ref15["velocity"]), mc.t(mc.difference_tolerance(ref15["velocity"])))
    want = MR.motion_rep(p, j)["rep15d"].clone()
    other = mc.make_inputs(9, 2, 40)
    p_in, j_in, out = p.clone(), j.clone(), torch.empty(2, 40, 55, 15, device=DEV)
    MR.motion_rep(p_in, j_in, out=out)                                                 # warm
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rep = MR.motion_rep(p_in, j_in, out=out)
    p_in.copy_(torch.from_numpy(other[0]))
    j_in.copy_(torch.from_numpy(other[1]))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(rep["rep15d"], MR.motion_rep(torch.from_numpy(other[0]).to(DEV), torch.from_numpy(other[1]).to(DEV))["rep15d"])
    p_in.copy_(p)
    j_in.copy_(j)
    before = torch.cuda.memory_allocated()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before and torch.equal(rep["rep15d"], want)
