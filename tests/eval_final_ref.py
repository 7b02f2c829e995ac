"""Float64 numpy statement of where evaluate.evaluate_final places the mesh of a run (utils/eval.py:343-344 and :389-399):

    E[k] = est_w2c[k] @ inv(c2w_0) @ P

est_w2c[k]: the estimated world-to-camera pose of frame k, relative to the first frame; c2w_0: the sequence's first ABSOLUTE
camera-to-world pose (eval_final opens the dataset with relative_pose=False); P: the ScanNet++ axis swap when the dataset is
ScanNet++, else the identity.  A camera-space point of frame k thus lands where the dataset's own world has it, and the mesh can
be compared with the dataset's ground-truth mesh.  numpy only; the inverse is numpy's general one, not the rigid closed form the
device uses."""
import numpy as np

SCANNETPP_SWAP = np.array([[0, 1, 0, 0], [-1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)  # eval.py:390-396
COMPENSATE_VECTOR = (-0.0 / 512.0, 2.5 / 512.0, -2.5 / 512.0)  # eval.py:461-462, scale = 1


def swap(dataset_name):
    """P of eval.py:389-398 (the comparison is case-insensitive here; the reference's own name is lower case)."""
    return SCANNETPP_SWAP if str(dataset_name).lower() == "scannetpp" else np.eye(4)


def placement(c2w_0, dataset_name):
    """F = inv(c2w_0) @ P, float64 [4,4]."""
    return np.linalg.inv(np.asarray(c2w_0, np.float64)) @ swap(dataset_name)


def mesh_extrinsics(est_w2cs, c2w_0, dataset_name):
    """E[k] = est_w2cs[k] @ F, float64 [K,4,4]."""
    return np.asarray(est_w2cs, np.float64) @ placement(c2w_0, dataset_name)


def compose_bound(*matrices):
    """The per-entry bound DESIGN.md 7.14 derives for frontend_ops.compose against float64: 16 * 2^-23 * max(1, max|entry|)^2."""
    m = max(float(np.abs(np.asarray(a, np.float64)).max()) for a in matrices)
    return 16 * 2.0 ** -23 * max(1.0, m) ** 2


def rigid(angle_deg, axis, translation):
    """A rigid 4x4 (float64): a rotation by angle_deg about the coordinate axis `axis` (0, 1, 2), then the translation."""
    a = np.radians(angle_deg)
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    M = np.eye(4)
    M[i, i], M[i, j], M[j, i], M[j, j] = c, -s, s, c
    M[:3, 3] = translation
    return M
