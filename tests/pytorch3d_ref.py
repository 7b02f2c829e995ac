"""pytorch3d's two published quaternion conversions, restated once for every reference under tests/ and for the PyTorch sides
of the map benches (scripts/benchlib.py).  Quaternions are (r, i, j, k).  Neither function imports or copies pytorch3d; both
work in the dtype and on the device of their input."""
import torch


def quaternion_to_matrix(q):
    """The published algorithm of pytorch3d.transforms.quaternion_to_matrix on [...,4] (what build_rotation calls,
    common_utils.py:44-45): entries scaled by 2 / |q|^2, the quaternion is NOT normalised first.  Returns [...,3,3]."""
    r, i, j, k = torch.unbind(q, -1)
    two_s = 2.0 / (q * q).sum(-1)
    o = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)), -1)
    return o.reshape(q.shape[:-1] + (3, 3))


def matrix_to_quaternion(m):
    """The published algorithm of pytorch3d.transforms.matrix_to_quaternion on [N,3,3] (what build_quaternion calls,
    common_utils.py:29-30): q_abs through _sqrt_positive_part (0 where the argument is not > 0, NaN included), four candidates,
    the one with the largest q_abs (first on ties), real part made >= 0.  Returns (quaternion [N,4], q_abs [N,4])."""
    m00, m01, m02 = m[:, 0, 0], m[:, 0, 1], m[:, 0, 2]
    m10, m11, m12 = m[:, 1, 0], m[:, 1, 1], m[:, 1, 2]
    m20, m21, m22 = m[:, 2, 0], m[:, 2, 1], m[:, 2, 2]
    arg = torch.stack([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22, 1.0 - m00 - m11 + m22], dim=-1)
    q_abs = torch.where(arg > 0, torch.sqrt(torch.where(arg > 0, arg, torch.ones_like(arg))), torch.zeros_like(arg))
    cand = torch.stack([
        torch.stack([q_abs[:, 0] ** 2, m21 - m12, m02 - m20, m10 - m01], dim=-1),
        torch.stack([m21 - m12, q_abs[:, 1] ** 2, m10 + m01, m02 + m20], dim=-1),
        torch.stack([m02 - m20, m10 + m01, q_abs[:, 2] ** 2, m12 + m21], dim=-1),
        torch.stack([m10 - m01, m20 + m02, m21 + m12, q_abs[:, 3] ** 2], dim=-1),
    ], dim=-2)
    cand = cand / (2.0 * q_abs[:, :, None].clamp(min=0.1))
    best = q_abs.argmax(dim=-1)
    q = cand[torch.arange(m.shape[0]), best]
    return torch.where(q[:, 0:1] < 0, -q, q), q_abs
