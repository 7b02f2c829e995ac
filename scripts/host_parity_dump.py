#!/usr/bin/env python
"""Prints one line per output tensor of the rasterizer library's host layer -- the case, the tensor's name and a sha256 over
its bytes -- so that two checkouts can be compared line for line (`--tree` names the checkout to import gaus_slam_amd from;
default: this one).  Only public names are used, with fixed seeds and the deterministic backward (the default backward sums
with float atomics and is not bit-stable from run to run), so equal lines mean equal bits: the operator with SH and with
precomputed colours, `lean` and the gradient sink, render_tracking (pose-only and full backward), the batched operator with
one and with K means2D carriers (forwards hashed, gradients compared with the per-frame operator: see batch_cases),
mark_visible, pose_quaternion, the fused losses (autograd nodes and *_loss_and_grads), FusedGaussianAdam and distCUDA2, on a
67x45 frame with 300 Gaussians and a 160x120 frame with 5 000.

Run each tree in a process of its own, under a time limit, e.g.
    timeout -k 10 120 python scripts/host_parity_dump.py > head.txt && timeout -k 10 120 python scripts/host_parity_dump.py --tree ../parent > parent.txt
"""
import argparse

import numpy as np
import torch

import benchlib

benchlib.import_tree(argparse.ArgumentParser())

from gaus_slam_amd import build, loss, rasterizer, render, scene_synth, tracking  # noqa: E402
from gaus_slam_amd.knn import distCUDA2  # noqa: E402
from gaus_slam_amd.optim import FusedGaussianAdam, GaussianSoA  # noqa: E402

LRS = dict(xyz=1e-3, opacity=5e-2, scaling=5e-3, rotation=1e-3, rgb=2.5e-3)
FIELDS = ("means3D", "opacities", "scales", "rotations", "colors")


def emit(case, **tensors):
    for name, t in tensors.items():
        print(f"{case} {name} {None if t is None else benchlib.tensor_digest(t)}", flush=True)


def leaves_of(sc, dev, requires_grad=True):
    out = {n: sc[n].to(dev).requires_grad_(requires_grad) for n in FIELDS}
    out["means2D"] = torch.zeros_like(out["means3D"], requires_grad=requires_grad)
    return out


def upstream(W, H, dev, seed):
    dc, da = scene_synth.make_upstream_grads(W, H, seed=seed)
    return dc.to(dev), da.to(dev)


def operator_cases(tag, sc, W, H, dev):
    dc, da = upstream(W, H, dev, 1)
    P = sc["means3D"].shape[0]
    g = torch.Generator().manual_seed(P)
    for name, sh_degree in (("colours", 0), ("sh", 1)):
        rs = render.settings_from_camera(sc["cam"], dev, sh_degree=sh_degree)
        lv = leaves_of(sc, dev)
        shs = (0.5 * torch.randn(P, 4, 3, generator=g)).to(dev).requires_grad_(True) if sh_degree else None
        pkg = render.render(rs, lv["means3D"], lv["means2D"], lv["opacities"], shs=shs, colors_precomp=None if sh_degree else lv["colors"],
                            scales=lv["scales"], rotations=lv["rotations"])
        emit(f"{tag} operator {name} forward", color=pkg["render_color"], radii=pkg["radius"], allmap=pkg["allmap"])
        torch.autograd.backward([pkg["render_color"], pkg["allmap"]], [dc, da])
        emit(f"{tag} operator {name} backward", shs=None if shs is None else shs.grad, **{n: t.grad for n, t in lv.items()})
        emit(f"{tag} mark_visible {name}", present=rasterizer.GaussianRasterizer(rs).markVisible(lv["means3D"].detach()))

    # the plain functions: every returned gradient, then `lean`, then the sink, and the sink through the autograd node
    rs = render.settings_from_camera(sc["cam"], dev)
    lv = leaves_of(sc, dev, requires_grad=False)
    e = torch.empty(0, dtype=torch.float32, device=dev)
    fwd = rasterizer.rasterize_gaussians(rs.bg, lv["means3D"], lv["colors"], lv["opacities"], lv["scales"], lv["rotations"], 1.0, e, rs.viewmatrix,
                                         rs.projmatrix, rs.tanfovx, rs.tanfovy, H, W, e, 0, rs.campos, True, False, False)
    R, radii, geom, binning, img = fwd[0], fwd[3], fwd[4], fwd[5], fwd[6]
    print(f"{tag} functions num_rendered {R}", flush=True)
    names = ("means2D", "colors", "opacities", "means3D", "transMat", "sh", "scales", "rotations")

    def backward(**kw):
        return rasterizer.rasterize_gaussians_backward(rs.bg, lv["means3D"], radii, lv["colors"], lv["scales"], lv["rotations"], 1.0, e, rs.viewmatrix,
                                                       rs.projmatrix, rs.tanfovx, rs.tanfovy, dc, da, e, 0, rs.campos, geom, R, binning, img,
                                                       True, False, **kw)
    emit(f"{tag} functions backward", **dict(zip(names, backward())))
    emit(f"{tag} functions backward lean", **dict(zip(names, backward(lean=True))))
    sink = {n: torch.full_like(lv[n], 7.0) for n in ("means3D", "opacities", "rotations")}
    res = backward(lean=True, grad_sink=sink)
    emit(f"{tag} functions backward sink", **dict(zip(names, res)), **{"sink_" + n: t for n, t in sink.items()})
    lv = leaves_of(sc, dev)
    views = {n: torch.full_like(lv[n], 3.0) for n in FIELDS}
    pkg = render.render(rs, lv["means3D"], lv["means2D"], lv["opacities"], colors_precomp=lv["colors"], scales=lv["scales"], rotations=lv["rotations"])
    with rasterizer.grad_sink(views):
        torch.autograd.backward([pkg["render_color"], pkg["allmap"]], [dc, da])
    emit(f"{tag} grad_sink context", **{"view_" + n: t for n, t in views.items()}, **{n: t.grad for n, t in lv.items()})


def tracking_cases(tag, W, H, P, dev):
    sc = scene_synth.make_scene(P, W, H, seed=3, regime="tracking")
    rs = render.settings_from_camera(sc["cam"], dev)
    dc, da = upstream(W, H, dev, 2)
    w2c0 = scene_synth.random_w2c(np.random.default_rng(5), max_rot_deg=2.0, max_trans=0.05).to(dev)
    emit(f"{tag} pose_quaternion", q=tracking.pose_quaternion(w2c0[:3, :4].contiguous()))
    for name, req in (("pose only", False), ("full", True)):
        w2c = w2c0.clone().requires_grad_(True)
        lv = {n: sc[n].to(dev).requires_grad_(req) for n in FIELDS}
        pkg = tracking.render_tracking(rs, w2c, lv["means3D"], lv["opacities"], lv["colors"], lv["scales"], lv["rotations"])
        emit(f"{tag} render_tracking {name} forward", color=pkg["render_color"], radii=pkg["radius"], allmap=pkg["allmap"])
        torch.autograd.backward([pkg["render_color"], pkg["allmap"]], [dc, da])
        emit(f"{tag} render_tracking {name} backward", w2c=w2c.grad, **{n: t.grad for n, t in lv.items()})
    return pkg


def batch_cases(tag, sc, W, H, dev, K=2):
    """The batched backward has no deterministic variant, so its float atomics make the gradients differ in the last bits
    from run to run: the forwards are hashed, each gradient is compared with the deterministic per-frame operator instead
    (relative to the gradient's largest entry; a different summation order moves it by ~1e-6, a wrong pointer by ~1)."""
    cams = [sc["cam"]] + [scene_synth.make_scene(8, W, H, seed=10 + k, regime="mapping")["cam"] for k in range(1, K)]
    settings = [render.settings_from_camera(c, dev) for c in cams]
    ups = [upstream(W, H, dev, 20 + k) for k in range(K)]
    ref = []
    for k in range(K):
        lv = leaves_of(sc, dev)
        pkg = render.render(settings[k], lv["means3D"], lv["means2D"], lv["opacities"], colors_precomp=lv["colors"], scales=lv["scales"],
                            rotations=lv["rotations"])
        torch.autograd.backward([pkg["render_color"], pkg["allmap"]], list(ups[k]))
        ref.append({n: t.grad for n, t in lv.items()})
    total = {n: sum(r[n] for r in ref) for n in ref[0]}
    close = lambda got, want: bool((got - want).abs().max() <= 1e-4 * want.abs().max())
    rasterizer.set_deterministic(False)
    try:
        for name, per_view in (("one carrier", False), ("K carriers", True)):
            lv = leaves_of(sc, dev)
            m2 = [torch.zeros_like(lv["means3D"], requires_grad=True) for _ in range(K)] if per_view else lv["means2D"]
            pkgs = render.render_batch(settings, lv["means3D"], m2, lv["opacities"], colors_precomp=lv["colors"], scales=lv["scales"],
                                       rotations=lv["rotations"])
            for k, pkg in enumerate(pkgs):
                emit(f"{tag} batch {name} forward frame {k}", color=pkg["render_color"], radii=pkg["radius"], allmap=pkg["allmap"])
            torch.autograd.backward([p["render_color"] for p in pkgs] + [p["allmap"] for p in pkgs], [u[0] for u in ups] + [u[1] for u in ups])
            checks = {n: close(lv[n].grad, total[n]) for n in FIELDS}
            if per_view:
                checks.update({f"means2D_{k}": close(m2[k].grad, ref[k]["means2D"]) for k in range(K)})
            else:
                checks["means2D"] = close(m2.grad, total["means2D"])
            for n, ok in checks.items():
                print(f"{tag} batch {name} backward {n} equals the per-frame operator to 1e-4: {ok}", flush=True)
    finally:
        rasterizer.set_deterministic(True)


def loss_cases(tag, pkg, W, H, dev):
    g = torch.Generator().manual_seed(W)
    gt_color, gt_depth = torch.rand(H, W, 3, generator=g).to(dev), (0.5 + 4.0 * torch.rand(H, W, 1, generator=g)).to(dev)
    color, allmap = pkg["render_color"].detach(), pkg["allmap"].detach()
    for name, node, fused, args in (("tracking", loss.tracking_loss, loss.tracking_loss_and_grads, (0.5, 1.0)),
                                    ("mapping", loss.mapping_loss, loss.mapping_loss_and_grads, (0.5, 1.0, 0.1))):
        c, a = color.clone().requires_grad_(True), allmap.clone().requires_grad_(True)
        value = node(c, a, gt_color, gt_depth, *args)
        (2.0 * value).backward()
        emit(f"{tag} {name}_loss", loss=value, g_color=c.grad, g_allmap=a.grad)
        value, g_color, g_allmap = fused(color, allmap, gt_color, gt_depth, *args)
        emit(f"{tag} {name}_loss_and_grads", loss=value, g_color=g_color, g_allmap=g_allmap)
    emit(f"{tag} mapping_loss_and_grads edge", **dict(zip(("loss", "g_color", "g_allmap"), loss.mapping_loss_and_grads(
        color, allmap, gt_color, gt_depth, 0.5, 1.0, 0.1, use_edge_growth=True, edge_thres=0.3, use_weight_norm=False))))


def adam_case(tag, sc, dev):
    P = sc["means3D"].shape[0]
    g = torch.Generator().manual_seed(P + 1)
    opt = FusedGaussianAdam(GaussianSoA({n: sc[n].to(dev) for n in FIELDS}), LRS)
    for it in range(3):
        opt.step((1e-2 * torch.randn(13 * P, generator=g)).to(dev))
        emit(f"{tag} adam step {it}", flat=opt.soa.flat, exp_avg=opt.exp_avg, exp_avg_sq=opt.exp_avg_sq)


def main():
    build.build()
    if not torch.cuda.is_available():
        print("# no GPU: nothing was run")
        return
    dev = torch.device("cuda", 0)
    rasterizer.set_deterministic(True)
    for W, H, P in ((67, 45, 300), (160, 120, 5000)):
        tag = f"{W}x{H} P={P}"
        sc = scene_synth.make_scene(P, W, H, seed=P, regime="mapping")
        operator_cases(tag, sc, W, H, dev)
        pkg = tracking_cases(tag, W, H, P, dev)
        batch_cases(tag, sc, W, H, dev)
        loss_cases(tag, pkg, W, H, dev)
        adam_case(tag, sc, dev)
    emit("distCUDA2 5000", dist2=distCUDA2(scene_synth.make_scene(5000, 160, 120, seed=9)["means3D"].to(dev)))
    emit("distCUDA2 0", dist2=distCUDA2(torch.empty(0, 3, device=dev)))


if __name__ == "__main__":
    main()
