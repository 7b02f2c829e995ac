"""Plain-PyTorch statement of densification from view-space gradients, as the yardstick of the densify_grad tests.

Written from the contract in include/gs2d_map.h (what scene/Gaussians.py:513-593 of the reference amounts to), step by step
on the INTERMEDIATE map -- append the clones, append the children, remove the split rows, prune everything that is left --
while carrying every row's source index and kind along.  That the result only depends on per-row decisions is therefore a
property this file checks, not one it assumes.  It neither imports nor copies the reference.

  classify(...)          float32, the dtype the reference decides in: every mask and the final (source, kind) list
  children(..., dtype)   the values of the children of split rows, in float32 or, on the same float32 inputs and the same
                         noise promoted exactly, in float64
"""
import torch

from tests.pytorch3d_ref import quaternion_to_matrix

OLD, CLONE, CHILD0, CHILD1 = 0, 1, 2, 3
SPLIT_DIV = 1.6  # 0.8 * N with N = 2


def thresholds(cfg):
    """(T, D, opacity_cull, scale_cull, M) as Python floats: products in double, M = 0.0 when scale_max is falsy."""
    cull = lambda k: cfg[k + "_cuil"] if k + "_cuil" in cfg else cfg[k + "_cull"]
    return (cfg["densify_grad_threshold"], cfg["percent_dense"] * cfg["extent"], cull("opacity"), cull("scale"),
            0.1 * cfg["extent"] if cfg["scale_max"] else 0.0)


def prune_mask(opacity_raw, scaling_raw, opacity_cull, scale_cull, M):
    """Step 4 on raw float32 [n] / [n,2] tensors: True where the row is removed."""
    e = torch.exp(scaling_raw)
    mask = (torch.sigmoid(opacity_raw) < opacity_cull) | (e.mean(dim=-1) < scale_cull)
    if M:
        mask = mask | (e.max(dim=1).values > M)
    return mask


def classify(opacities, scales, accum, denom, T, D, opacity_cull, scale_cull, M):
    """opacities [P,1], scales [P,2], accum [P], denom [P]: float32 CPU tensors.  Returns a dict with
    g [P]; clone, split [P] bool (step 2 / 3 selections); src, kind: int64 lists of the final rows (source row, OLD / CLONE /
    CHILD0 / CHILD1); n_cloned, n_split, n_pruned, P_new; child_pruned [P] bool (split rows whose children are removed);
    old_pruned [P] bool (what step 4 decides for the row's own values)."""
    assert T > 0
    P = opacities.shape[0]
    o, s = opacities[:, 0].float(), scales.float()
    g = accum / denom                                           # step 1
    g[g.isnan()] = 0.0
    sel = g >= T
    big = torch.exp(s).max(dim=1).values
    clone = sel & (big <= D)                                    # step 2: appended unchanged
    src = torch.arange(P)
    o_all, s_all = torch.cat([o, o[clone]]), torch.cat([s, s[clone]])
    src_all = torch.cat([src, src[clone]])
    kind_all = torch.cat([torch.full((P,), OLD), torch.full((int(clone.sum()),), CLONE)])
    split = sel & (big > D)                                     # step 3: the clones carry no gradient (T > 0), they never split
    n_split = int(split.sum())
    child_s = torch.log(torch.exp(s[split]) / SPLIT_DIV)
    o_all = torch.cat([o_all, o[split].repeat(2)])
    s_all = torch.cat([s_all, child_s.repeat(2, 1)])
    src_all = torch.cat([src_all, src[split].repeat(2)])
    kind_all = torch.cat([kind_all, torch.full((n_split,), CHILD0), torch.full((n_split,), CHILD1)])
    removed = torch.cat([split, torch.zeros(o_all.shape[0] - P, dtype=torch.bool)])
    o_all, s_all, src_all, kind_all = o_all[~removed], s_all[~removed], src_all[~removed], kind_all[~removed]
    pr = prune_mask(o_all, s_all, opacity_cull, scale_cull, M)  # step 4: every row of the intermediate map
    src_f, kind_f = src_all[~pr], kind_all[~pr]
    child_pruned = torch.zeros(P, dtype=torch.bool)
    child_pruned[src_all[pr & (kind_all == CHILD0)]] = True
    n_cloned = int(clone.sum())
    return dict(g=g, clone=clone, split=split, src=src_f, kind=kind_f, n_cloned=n_cloned, n_split=n_split,
                n_pruned=int(pr.sum()), P_new=int(src_f.shape[0]), child_pruned=child_pruned,
                old_pruned=prune_mask(o, s, opacity_cull, scale_cull, M))


def children(means3D, scales, rotations, noise, rows, dtype):
    """The two children of each of `rows` (int64 [n], source rows that split).  means3D [P,3], scales [P,2], rotations [P,4],
    noise [P,2,2] (row, copy, axis): float32, promoted to `dtype`; 1.6 enters as the float32 value the reference divides by.
    Returns dict(means3D [n,2,3], scales [n,2], offset [n,2,3], R [n,3,3], samples [n,2,3]: the local
    offsets (e0 n0, e1 n1, 0))."""
    e = torch.exp(scales[rows].to(dtype))
    R = quaternion_to_matrix(rotations[rows].to(dtype))
    n = rows.shape[0]
    samples = torch.cat([e[:, None, :] * noise[rows].to(dtype), torch.zeros(n, 2, 1, dtype=dtype)], dim=-1)   # [n,copy,3]
    offset = torch.einsum("nab,ncb->nca", R, samples)
    div = torch.tensor(SPLIT_DIV, dtype=torch.float32).to(dtype)
    return dict(means3D=offset + means3D[rows].to(dtype)[:, None, :], scales=torch.log(e / div), offset=offset, R=R,
                samples=samples)


# The ordering example of the host test: one row per class.  D = 0.02, M = 0.2, T = 2e-4, opacity_cull = 0.05, scale_cull = 5e-4.
#   0 kept (no gradient)            1 pruned (transparent)           2 cloned, both kept          3 cloned, both pruned (transparent)
#   4 split, children kept          5 split, parent larger than M, children (0.3 / 1.6 < 0.2) kept
def example_map():
    lg = lambda *v: torch.log(torch.tensor(v))
    scales = torch.stack([lg(0.01, 0.01), lg(0.01, 0.01), lg(0.01, 0.015), lg(0.01, 0.015), lg(0.05, 0.03), lg(0.3, 0.1)])
    opacities = torch.tensor([[2.0], [-6.0], [1.0], [-6.0], [0.5], [3.0]])
    accum = torch.tensor([0.0, 0.0, 9e-4, 9e-4, 5e-4, 1e-3])
    denom = torch.tensor([0.0, 2.0, 3.0, 3.0, 1.0, 2.0])
    cfg = dict(densify_grad_threshold=2e-4, percent_dense=0.01, extent=2.0, opacity_cuil=0.05, scale_cuil=5e-4, scale_max=0.1)
    src = [0, 2, 2, 4, 5, 4, 5]
    kind = [OLD, OLD, CLONE, CHILD0, CHILD0, CHILD1, CHILD1]
    return opacities, scales, accum, denom, cfg, src, kind
