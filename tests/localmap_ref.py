"""Plain-PyTorch restatement of the reference's hand-over of a local map to the global map, as the yardstick of the localmap
tests: Backend.transfer_map_params (slam/Backend.py:158-161), the opacity clamp (:226) and what Gaussians.add_params appends.

It neither imports nor copies the reference.  pytorch3d's quaternion_to_matrix and matrix_to_quaternion are those of
tests/pytorch3d_ref.py.  Everything takes `dtype` and works on any
device, so that the same code is the float32 formulation (on the CPU or on the GPU) and, on the same float32 inputs promoted
exactly, its float64 evaluation.  The inputs every localmap test uses are generated here too, once per size."""
import functools
import math

import numpy as np
import torch

from tests.pytorch3d_ref import matrix_to_quaternion, quaternion_to_matrix  # noqa: F401  (ref.quaternion_to_matrix in the tests)
from tests.util import qdiff  # noqa: F401  (ref.qdiff in the tests)

F32 = np.float32


# ------------------------------------------------------------------------------------------------------------------ formulas
def transfer_map_params(xyz, rotation, transfer):
    """Backend.py:159-160 on tensors of one dtype and device.  Returns (xyz [n,3], rotation [n,4])."""
    new_xyz = (transfer[:3, :3] @ xyz.T + transfer[:3, 3:]).T                                   # :159
    new_rot = matrix_to_quaternion(torch.matmul(transfer[None, :3, :3], quaternion_to_matrix(rotation)))[0]  # :160
    return new_xyz, new_rot


def quaternion_multiply(a, b):
    """Hamilton product of [N,4] quaternions (w,x,y,z): the rotation of a, after that of b."""
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack((aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw), -1)


def rotation_by_quaternion_product(rotation, transfer):
    """The other route the contract allows: matrix_to_quaternion(R_t), then a quaternion product with q / |q|."""
    qt = matrix_to_quaternion(transfer[None, :3, :3])[0]
    return quaternion_multiply(qt.expand_as(rotation), rotation / rotation.norm(dim=-1, keepdim=True))


def orthonormality_error(transfer):
    """max |R_t R_t^T - I| of a float32 transfer, evaluated in float64."""
    R = transfer[:3, :3].double()
    return float((R @ R.T - torch.eye(3, dtype=torch.float64)).abs().max())


def merged_rows(params, transfer, cap, dtype):
    """What rows [P,P+n) of the merged map hold (Backend.py:225-227), evaluated in `dtype` on float32 inputs; opacities stay
    float32: torch.min picks one of its two inputs."""
    xyz, rot = transfer_map_params(params["means3D"].to(dtype), params["rotations"].to(dtype), transfer.to(dtype))
    opac = torch.minimum(params["opacities"], torch.full_like(params["opacities"], cap))        # :226
    return dict(means3D=xyz, opacities=opac, scales=params["scales"], rotations=rot, colors=params["colors"])


def means_bound(xyz, transfer):
    """8 * 2^-24 * (|R| |x| + |t|): the rounding of the six float32 operations of ((r0 x + r1 y) + r2 z) + t, the bound
    tests/test_gpu_densify.py uses for its means."""
    T = transfer.double()
    return 8 * 2.0 ** -24 * (xyz.double().abs() @ T[:3, :3].abs().T + T[:3, 3].abs())


# -------------------------------------------------------------------------------------------------------------------- inputs
def _rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = math.radians(deg)
    return np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * K @ K


def _pose(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


# the two float32 poses whose inv(A) @ B is one of the transfers; the product is formed by whoever is under test
POSE_A = torch.from_numpy(_pose(_rot((0.2, 0.9, -0.4), 63.0), (1.3, -0.2, 0.8)).astype(F32))
POSE_B = torch.from_numpy(_pose(_rot((-0.7, 0.1, 0.6), 141.0), (-0.5, 0.9, 2.1)).astype(F32))

TRANSFER_NAMES = ["identity", "general", "pi_x", "pi_y", "pi_z", "skew_179.9", "inv_a_b"]


@functools.lru_cache(maxsize=None)
def transfer(name):
    """float32 [4,4] CPU tensor.  "inv_a_b" here is the float32 CPU product; the GPU tests replace it with what
    localmap.transfer_matrix forms from POSE_A and POSE_B on the device."""
    t = (0.4, -1.1, 0.7)
    if name == "identity":
        T = np.eye(4)
    elif name == "general":
        T = _pose(_rot((0.3, -0.8, 0.5), 37.0), t)
    elif name in ("pi_x", "pi_y", "pi_z"):  # exact in float32: each exercises another branch of matrix_to_quaternion
        d = {"pi_x": (1, -1, -1), "pi_y": (-1, 1, -1), "pi_z": (-1, -1, 1)}[name]
        T = _pose(np.diag(np.asarray(d, np.float64)), t)
    elif name == "skew_179.9":
        T = _pose(_rot((0.55, -0.35, 0.76), 179.9), t)
    else:
        return (torch.linalg.inv(POSE_A) @ POSE_B).contiguous()
    return torch.from_numpy(T.astype(F32))


@functools.lru_cache(maxsize=None)
def incoming(n, cap, seed=0):
    """A local map of n rows (float32 CPU, fields are views of one flat [13 n] buffer as in a GaussianSoA): raw quaternions with
    |q| from 1e-3 to 1e3, half of them with a negative real part, every seventh an exact identity; opacity logits equal to
    `cap`, below it and above it in turn."""
    g = torch.Generator().manual_seed(1000 * n + seed)
    q = torch.randn(n, 4, generator=g)
    q = q / q.norm(dim=-1, keepdim=True) * 10.0 ** (6 * torch.rand(n, 1, generator=g) - 3)
    row = torch.arange(n)
    q[:, 0] = torch.where(row % 2 == 1, -q[:, 0].abs(), q[:, 0].abs())
    q[row % 7 == 3] = torch.tensor([1.0, 0.0, 0.0, 0.0])
    o = torch.full((n, 1), cap) + torch.where((row % 3 == 1)[:, None], -3 * torch.rand(n, 1, generator=g) - 1e-3,
                                               5 * torch.rand(n, 1, generator=g) + 1e-3)
    o[row % 3 == 0] = cap
    fields = dict(means3D=3 * torch.randn(n, 3, generator=g), opacities=o, scales=torch.log(0.005 + 0.3 * torch.rand(n, 2, generator=g)),
                  rotations=q, colors=torch.rand(n, 3, generator=g))
    flat = torch.cat([fields[k].reshape(-1) for k in ("means3D", "opacities", "scales", "rotations", "colors")])
    out, off = {}, 0
    for k, w in (("means3D", 3), ("opacities", 1), ("scales", 2), ("rotations", 4), ("colors", 3)):
        out[k] = flat[off:off + w * n].view(n, w)
        off += w * n
    return out
