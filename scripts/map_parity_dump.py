#!/usr/bin/env python
"""Prints one line per case of the map layer -- the case name and a sha256 over the bytes of every output buffer -- so that two
checkouts can be compared line for line (`--tree` names the checkout to import gaus_slam_amd from; default: this one).  Only
the public Python API is used (and _map_lib.lib() for the three *_ws_bytes queries), with fixed seeds, so equal lines mean
equal bits: seeding, pruning, densification statistics and densify_and_prune, merge_local_map, the raw-parameter mapping step,
the pose optimiser and frame_stats, the evaluation metrics, the TSDF volume with its mesh and the reconstruction metrics, at
sizes with ragged last blocks and odd row counts.

The first two blocks need no GPU: the workspace sizes, and one line per refused call -- a fixed list of bad arguments (wrong
type, dtype, shape, stride, CPU tensor, out-of-range scalar) for every public function of the layer, with the RuntimeError's
text or ACCEPTED, so that two trees refuse the same inputs in the same words.  The library is stubbed there (nothing may get as
far as a call) and a tensor subclass that claims to be a CUDA tensor carries well-formed arguments past the device checks.
Without a GPU the script stops after these blocks.  Run each tree in a process of its own, under a time limit, e.g.
    timeout -k 10 300 python scripts/map_parity_dump.py > head.txt && timeout -k 10 300 python scripts/map_parity_dump.py --tree ../parent > parent.txt
"""
import argparse
import math

import torch

import benchlib
from benchlib import DENSIFY

benchlib.import_tree(argparse.ArgumentParser())

from gaus_slam_amd import _map_lib, build, densify, evaluate, localmap, mapping, pose, recon, tsdf  # noqa: E402
from gaus_slam_amd.optim import FusedGaussianAdam, GaussianSoA  # noqa: E402

LRS = dict(xyz=1e-3, opacity=5e-2, scaling=5e-3, rotation=1e-3, rgb=2.5e-3)


def emit(name, *tensors):
    print(f"{name} {benchlib.tensor_digest(*tensors)}", flush=True)


def map_buffers(opt):
    return opt.soa.flat, opt.exp_avg, opt.exp_avg_sq


def make_fields(P, g):
    rn = lambda *s: torch.randn(*s, generator=g)
    return dict(means3D=2.0 * rn(P, 3), opacities=2.0 * rn(P, 1), scales=math.log(0.02) + 1.5 * rn(P, 2), rotations=rn(P, 4) + 0.2,
                colors=torch.rand(P, 3, generator=g))


def make_opt(P, dev, seed, cls=FusedGaussianAdam, activated=False):
    g = torch.Generator().manual_seed(seed)
    f = make_fields(P, g)
    if activated:
        f["opacities"], f["scales"] = torch.sigmoid(f["opacities"]), f["scales"].exp()
    opt = cls(GaussianSoA({k: v.to(dev) for k, v in f.items()}), LRS)
    benchlib.seeded_moments(opt, g)
    return opt, g


def make_frame(W, H, dev, seed):
    g = torch.Generator().manual_seed(seed)
    alpha = torch.rand(H, W, generator=g)
    depth = 0.5 + 4.0 * torch.rand(H, W, generator=g)
    gt_depth = depth + 0.3 * torch.randn(H, W, generator=g)
    gt_depth[torch.rand(H, W, generator=g) < 0.05] = 0.0          # holes: the validity mask and its 3x3 erosion
    gt_depth[torch.rand(H, W, generator=g) < 0.02] = 20.0
    allmap = torch.randn(7, H, W, generator=g)
    allmap[0], allmap[1] = depth * alpha, alpha
    gt_color = torch.rand(H, W, 3, generator=g)
    intrinsics = torch.tensor([[0.9 * W, 0.0, 0.5 * W - 0.5], [0.0, 0.95 * W, 0.5 * H - 0.5], [0.0, 0.0, 1.0]])
    return allmap.to(dev), gt_color.to(dev), gt_depth.to(dev), intrinsics


def rigid(deg, axis, t, dev):
    a = torch.tensor(axis, dtype=torch.float64)
    a = a / a.norm()
    K = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=torch.float64)
    m = torch.eye(4, dtype=torch.float64)
    m[:3, :3] = torch.eye(3, dtype=torch.float64) + math.sin(math.radians(deg)) * K + (1 - math.cos(math.radians(deg))) * K @ K
    m[:3, 3] = torch.tensor(t, dtype=torch.float64)
    return m.float().contiguous().to(dev)


def host_block():
    L = _map_lib.lib()
    for W, H in ((1, 1), (32, 32), (67, 45), (640, 480)):
        print(f"seed_ws_bytes {W}x{H} {L.gs2d_map_seed_ws_bytes(W, H)}")
    for P in (0, 1, 1023, 1024, 1025, 200003):
        print(f"prune_ws_bytes {P} {L.gs2d_map_prune_ws_bytes(P)}")
        print(f"densify_ws_bytes {P} {L.gs2d_map_densify_ws_bytes(P)}", flush=True)


class _Reached(Exception):
    """Raised by the stubbed library: every check before the first library call has passed."""


class _Dev(torch.Tensor):
    is_cuda = True  # a host tensor that passes for a device tensor: what lies behind the device checks is reached on any machine


def _reached(*a, **k):
    raise _Reached()


def _cpu_opt(cls=FusedGaussianAdam, P=5):
    return cls(GaussianSoA(dict(means3D=torch.zeros(P, 3), opacities=torch.zeros(P, 1), scales=torch.zeros(P, 2),
                                rotations=torch.ones(P, 4), colors=torch.zeros(P, 3))), {})


def refusal_cases():
    """[(name, thunk)]: host tensors only; `on` marks one as a device tensor."""
    on = lambda t: t.as_subclass(_Dev)
    z, eye = torch.zeros, torch.eye
    cases = []
    add = lambda name, fn, *a, **k: cases.append((name, lambda: fn(*a, **k)))

    # ---- densify: one frame
    H, W = 6, 8
    allmap, col, dep, K, w2c = z(7, H, W), z(H, W, 3), torch.ones(H, W), eye(3), eye(4)
    frame = dict(allmap=allmap, gt_color=col, gt_depth=dep, intrinsics=K, w2c=w2c, sil_thres=0.5)
    dev_frame = dict(frame, allmap=on(allmap), gt_color=on(col), gt_depth=on(dep), w2c=on(w2c))
    for what, change in (("cpu", {}), ("allmap 6 planes", dict(allmap=allmap[:6])), ("allmap float64", dict(allmap=allmap.double())),
                         ("allmap strided", dict(allmap=allmap.permute(0, 2, 1).contiguous().permute(0, 2, 1))),
                         ("allmap list", dict(allmap=[[0.0]])), ("allmap none", dict(allmap=None)),
                         ("gt_color chw", dict(gt_color=col.permute(2, 0, 1).contiguous())), ("gt_color half", dict(gt_color=col.half())),
                         ("gt_depth narrow", dict(gt_depth=dep[:, :-1])), ("gt_depth strided", dict(gt_depth=dep.t().contiguous().t())),
                         ("gt_depth float64", dict(gt_depth=dep.double())), ("gt_depth numpy", dict(gt_depth=dep.numpy())),
                         ("intrinsics 4x4", dict(intrinsics=eye(4))), ("mode", dict(mode="random")), ("no sil_thres", dict(sil_thres=None)),
                         ("mode all cpu", dict(allmap=None, mode="all")), ("edge no allmap", dict(allmap=None, mode="edge"))):
        add(f"seed_from_frame {what}", densify.seed_from_frame, **{**frame, **change})
    for what, change in (("well-formed", {}), ("gt_color on cpu", dict(gt_color=col)), ("gt_depth on cpu", dict(gt_depth=dep)),
                         ("w2c on cpu", dict(w2c=w2c)), ("w2c 3x3", dict(w2c=on(eye(3)))), ("shape before device", dict(gt_color=col[:, :-1])),
                         ("mode all", dict(allmap=None, mode="all"))):
        add(f"seed_from_frame device {what}", densify.seed_from_frame, **{**dev_frame, **change})
    add("seed_select cpu", densify.seed_select, allmap, dep, sil_thres=0.5)
    add("seed_select mode", densify.seed_select, allmap, dep, mode="random", sil_thres=0.5)
    add("seed_select no sil_thres", densify.seed_select, allmap, dep, mode="edge")
    add("seed_select all cpu", densify.seed_select, None, dep, mode="all")
    add("seed_select device", densify.seed_select, on(allmap), on(dep), sil_thres=0.5)
    add("seed_median of edge", densify.seed_median, densify.SeedSelection(0, None, "edge", W, H))
    sel = densify.SeedSelection(3, on(z(64, dtype=torch.uint8)), "splatam", W, H)
    out = {"means3D": on(z(3, 3)), "opacities": on(z(3, 1)), "scales": on(z(3, 2)), "rotations": on(z(3, 4)), "colors": on(z(3, 3))}
    write = dict(sel=sel, allmap=on(allmap), gt_color=on(col), gt_depth=on(dep), intrinsics=K, c2w=on(w2c), out=out)
    for what, change in (("well-formed", {}), ("other size", dict(sel=sel._replace(width=W + 1))), ("out rows", dict(out=dict(out, scales=on(z(4, 2))))),
                         ("out on cpu", dict(out=dict(out, colors=z(3, 3)))), ("pixel_index int64", dict(pixel_index=on(z(3, dtype=torch.int64)))),
                         ("c2w float64", dict(c2w=on(w2c.double()))), ("c2w on cpu", dict(c2w=w2c)), ("frame on cpu", dict(gt_color=col))):
        add(f"seed_write {what}", densify.seed_write, **{**write, **change})
    add("c2w_from_w2c cpu", densify.c2w_from_w2c, w2c)
    add("c2w_from_w2c 3x3", densify.c2w_from_w2c, eye(3))
    cfg = dict(sil_thres=0.5, opacity_cuil=0.005, scale_cuil=1e-4, scale_max=1.0)
    add("prune_gaussians cpu", densify.prune_gaussians, _cpu_opt(), 0.005, 1e-4, 1.0)
    add("add_new_gaussians cpu", densify.add_new_gaussians, _cpu_opt(), allmap, col, dep, K, w2c, cfg, {})

    # ---- densify: statistics and densify_and_prune
    opt = _cpu_opt()
    stats = densify.DensificationStats(opt)
    r, g = torch.ones(5, dtype=torch.int32), z(5, 3)
    for what, args in (("cpu", (r, g)), ("radii int64", (r.long(), g)), ("radii rows", (r[:4], g)), ("radii strided", (torch.ones(10, dtype=torch.int32)[::2], g)),
                       ("grad float64", (r, g.double())), ("grad columns", (r, g[:, :2])), ("grad strided", (r, z(3, 5).t())),
                       ("grad numpy", (r, g.numpy()))):
        add(f"stats.add {what}", stats.add, *args)
    add("densify_and_prune cpu", densify.densify_and_prune, opt, stats, DENSIFY)
    for what, change in (("T zero", dict(densify_grad_threshold=0.0)), ("T underflows", dict(densify_grad_threshold=1e-50)),
                         ("T negative", dict(densify_grad_threshold=-1.0)), ("extent zero", dict(extent=0.0)), ("extent inf", dict(extent=float("inf")))):
        add(f"densify_and_prune {what}", densify.densify_and_prune, opt, stats, dict(DENSIFY, **change))
    add("densify_and_prune lacks percent_dense", densify.densify_and_prune, opt, stats, {k: v for k, v in DENSIFY.items() if k != "percent_dense"})
    add("densify_and_prune foreign stats", densify.densify_and_prune, opt, densify.DensificationStats(_cpu_opt()), DENSIFY)

    # ---- localmap
    good = dict(means3D=z(6, 3), opacities=z(6, 1), scales=z(6, 2), rotations=torch.ones(6, 4), colors=z(6, 3))
    for what, change in (("cpu", {}), ("field missing", dict(params={k: v for k, v in good.items() if k != "colors"})),
                         ("params list", dict(params=list(good.values()))), ("scales rows", dict(params=dict(good, scales=good["scales"][:5]))),
                         ("rotations columns", dict(params=dict(good, rotations=good["rotations"][:, :3].contiguous()))),
                         ("colors float64", dict(params=dict(good, colors=good["colors"].double()))),
                         ("means3D strided", dict(params=dict(good, means3D=good["means3D"].t().contiguous().t()))),
                         ("opacities strided", dict(params=dict(good, opacities=z(6, 2)[:, :1]))), ("transfer 3x3", dict(transfer=eye(3))),
                         ("transfer batched", dict(transfer=eye(4)[None])), ("transfer float64", dict(transfer=eye(4, dtype=torch.float64))),
                         ("transfer strided", dict(transfer=eye(8)[::2, ::2])), ("opacity_cap 1.5", dict(opacity_cap=1.5)),
                         ("opacity_cap 0", dict(opacity_cap=0.0))):
        add(f"merge_local_map {what}", localmap.merge_local_map, _cpu_opt(mapping.RawGaussianAdam), **{**dict(params=good, transfer=eye(4)), **change})
    add("merge_local_map cpu activated", localmap.merge_local_map, _cpu_opt(), good, eye(4), activated=True)
    create = dict(gt_color=col, gt_depth=dep, intrinsics=K, lrs={})
    for what, change in (("cpu", {}), ("cpu with w2c", dict(w2c=w2c)), ("gt_color chw", dict(gt_color=col.permute(2, 0, 1).contiguous())),
                         ("gt_color half", dict(gt_color=col.half())), ("gt_depth narrow", dict(gt_depth=dep[:, :-1])),
                         ("gt_depth strided", dict(gt_depth=dep.t().contiguous().t())), ("gt_depth float64", dict(gt_depth=dep.double())),
                         ("gt_depth flat", dict(gt_depth=torch.ones(H * W))), ("intrinsics 4x4", dict(intrinsics=eye(4))),
                         ("device", dict(gt_color=on(col), gt_depth=on(dep))), ("device, gt_color on cpu", dict(gt_depth=on(dep)))):
        add(f"create_map {what}", localmap.create_map, **{**create, **change})
    add("transfer_matrix cpu", localmap.transfer_matrix, eye(4), eye(4))
    add("transfer_matrix 3x3", localmap.transfer_matrix, eye(3), eye(4))
    add("transfer_matrix ref2f0 on cpu", localmap.transfer_matrix, on(eye(4)), eye(4))
    add("transfer_matrix ref2f0 list", localmap.transfer_matrix, on(eye(4)), [[1.0]])
    add("opacity_cap_value 1", localmap.opacity_cap_value, 1.0)

    # ---- mapping
    raw = _cpu_opt(mapping.RawGaussianAdam)
    add("RawGaussianAdam.render_leaves cpu", raw.render_leaves)
    add("RawGaussianAdam.step cpu", raw.step, z(13 * 5))
    add("map_frames other optimiser", mapping.map_frames, _cpu_opt(), [(None, None, None)], 1, 0.5, 1.0, 0.0)
    add("map_frames no frames", mapping.map_frames, raw, [], 1, 0.5, 1.0, 0.0)
    add("map_frames short order", mapping.map_frames, raw, [(None, None, None)], 3, 0.5, 1.0, 0.0, order=[0])
    add("map_frames densify_interval alone", mapping.map_frames, raw, [(None, None, None)], 1, 0.5, 1.0, 0.0, densify_interval=2)

    # ---- pose
    P = pose.PoseOptimizer
    add("PoseOptimizer cpu", P, eye(4))
    add("PoseOptimizer 3x3", P, eye(3))
    add("PoseOptimizer float64", P, eye(4, dtype=torch.float64))
    add("PoseOptimizer strided", P, eye(4).t() + z(4, 4).t())
    add("PoseOptimizer list", P, [[1.0]])
    add("PoseOptimizer left on cpu", P, None, left=eye(4), device="cuda:0")
    add("PoseOptimizer device cpu", P, None, device="cpu")
    add("PoseOptimizer lr key missing", P, None, {k: 1e-3 for k in pose.LR_KEYS if k != "cam_trans_lr_final"}, device="cuda:0")
    add("PoseOptimizer max_step 0", P, None, dict(pose.DEFAULT_LR, cam_rot_lr_max_step=0), device="cuda:0")
    add("PoseOptimizer beta 1", P, None, betas=(0.9, 1.0), device="cuda:0")
    add("PoseOptimizer eps negative", P, None, eps=-1.0, device="cuda:0")
    add("frame_stats cpu", pose.frame_stats, z(7, 4, 5), z(4, 5))
    add("frame_stats 6 planes", pose.frame_stats, z(6, 4, 5), z(4, 5))
    add("frame_stats gt_depth float64", pose.frame_stats, on(z(7, 4, 5)), on(z(4, 5).double()))
    add("frame_stats gt_depth on cpu", pose.frame_stats, on(z(7, 4, 5)), z(4, 5))
    add("frame_stats device", pose.frame_stats, on(z(7, 4, 5)), on(z(4, 5)))
    add("track other optimiser", pose.track, None, object(), *([None] * 9), 1)

    # ---- evaluate
    H, W = 171, 200
    ok = dict(color=z(3, H, W), allmap=z(7, H, W), gt_color=z(H, W, 3), gt_depth=z(H, W))
    okd = {k: on(v) for k, v in ok.items()}
    n_out = evaluate.EVAL_OUT_DOUBLES
    for what, kw in (("cpu", ok), ("6 planes", dict(ok, allmap=z(6, H, W))), ("color hwc", dict(ok, color=z(H, W, 3))),
                     ("gt_color chw", dict(ok, gt_color=z(3, H, W))), ("color float64", dict(ok, color=z(3, H, W, dtype=torch.float64))),
                     ("color strided", dict(ok, color=z(3, W, H).transpose(1, 2))), ("gt_depth wide", dict(ok, gt_depth=z(H, W + 1))),
                     ("out float32", dict(ok, out=z(n_out))), ("out long", dict(ok, out=z(n_out + 1, dtype=torch.float64))),
                     ("out strided", dict(ok, out=z(2 * n_out, dtype=torch.float64)[::2])), ("out list", dict(ok, out=[0.0] * n_out)),
                     ("ws float32", dict(ok, ws=z(64))), ("ws 2-d", dict(ok, ws=z(8, 8, dtype=torch.uint8))),
                     ("ws strided", dict(ok, ws=z(64, dtype=torch.uint8)[::2])),
                     ("device", okd), ("device, color on cpu", dict(okd, color=ok["color"])),
                     ("device, out on cpu", dict(okd, out=z(n_out, dtype=torch.float64))), ("device, ws on cpu", dict(okd, ws=z(64, dtype=torch.uint8))),
                     ("device, ws dtype before out device", dict(okd, out=z(n_out, dtype=torch.float64), ws=z(64)))):
        add(f"frame_metrics {what}", evaluate.frame_metrics, **kw)
    for h, w in ((160, 400), (400, 160), (100, 100)):
        add(f"frame_metrics {w}x{h}", evaluate.frame_metrics, z(3, h, w), z(7, h, w), z(h, w, 3), z(h, w))
    frames = [(None, None, None)] * 3
    add("evaluate_map no frames", evaluate.evaluate_map, {}, [])
    add("evaluate_map tsdf without intrinsics", evaluate.evaluate_map, {}, frames, tsdf=object())
    add("evaluate_map mesh_interval 0", evaluate.evaluate_map, {}, frames, tsdf=object(), mesh_intrinsics=(1, 1, 0, 0), mesh_interval=0)
    add("evaluate_map one extrinsic", evaluate.evaluate_map, {}, frames, tsdf=object(), mesh_intrinsics=(1, 1, 0, 0), mesh_extrinsics=[eye(4)])
    add("evaluate_map one pose list", evaluate.evaluate_map, {}, frames, est_w2cs=[eye(4)])
    add("evaluate_map cpu", evaluate.evaluate_map, dict(means3D=z(5, 3)), frames)
    add("ate_rmse shapes", evaluate.ate_rmse, z(3, 4, 4), z(2, 4, 4))
    add("ate_rmse no finite pose", evaluate.ate_rmse, z(2, 4, 4), torch.full((2, 4, 4), float("nan")))

    # ---- tsdf
    V = tsdf.TSDFVolume
    for what, change in (("dims 1", dict(dims=(1, 5, 5))), ("two dims", dict(dims=(5, 5))), ("2^31 voxels", dict(dims=(2048, 1024, 1024))),
                         ("voxel_length 0", dict(voxel_length=0.0)), ("sdf_trunc negative", dict(sdf_trunc=-1.0)),
                         ("depth_trunc 0", dict(depth_trunc=0.0)), ("origin inf", dict(origin=(0.0, float("inf"), 0.0)))):
        add(f"TSDFVolume {what}", V, **{**dict(origin=(0, 0, 0), dims=(4, 4, 4), device="cpu"), **change})
    add("TSDFVolume.from_bounds flat", V.from_bounds, (0, 0, 0), (1, 0, 1), device="cpu")
    add("bounds_of_map 1-d", tsdf.bounds_of_map, z(3))
    H, W = 12, 16
    vol = V((0, 0, 0), (4, 4, 4), device="cpu")
    vold = V((0, 0, 0), (4, 4, 4), device="cpu")
    vold.planes = on(vold.planes)
    ok = dict(color=z(3, H, W), depth=z(H, W), intrinsics=(10.0, 10.0, 8.0, 6.0), w2c=eye(4))
    okd = dict(ok, color=on(ok["color"]), depth=on(ok["depth"]), w2c=on(ok["w2c"]))
    for what, kw in (("cpu", ok), ("depth 3-d", dict(ok, depth=z(1, H, W))), ("color hwc", dict(ok, color=z(H, W, 3))),
                     ("depth float64", dict(ok, depth=z(H, W, dtype=torch.float64))), ("color strided", dict(ok, color=z(3, W, H).transpose(1, 2))),
                     ("w2c 3x3", dict(ok, w2c=eye(3))), ("w2c float64", dict(ok, w2c=eye(4, dtype=torch.float64))),
                     ("three intrinsics", dict(ok, intrinsics=(10.0, 10.0, 8.0))), ("fx 0", dict(ok, intrinsics=(0.0, 10.0, 8.0, 6.0))),
                     ("cx nan", dict(ok, intrinsics=(10.0, 10.0, float("nan"), 6.0))), ("3x3 intrinsics, cpu", dict(ok, intrinsics=K * 10.0))):
        add(f"TSDFVolume.integrate {what}", vol.integrate, **kw)
    add("TSDFVolume.integrate device intrinsics", vold.integrate, **dict(okd, intrinsics=on(K * 10.0)))
    add("TSDFVolume.integrate device", vold.integrate, **okd)
    add("TSDFVolume.integrate device, volume on cpu", vol.integrate, **okd)
    add("TSDFVolume.integrate device, w2c on cpu", vold.integrate, **dict(okd, w2c=eye(4)))
    render = dict(render_color=ok["color"], allmap=z(7, H, W), intrinsics=ok["intrinsics"], w2c=ok["w2c"])
    add("TSDFVolume.integrate_render cpu", vol.integrate_render, **render)
    add("TSDFVolume.integrate_render 6 planes", vol.integrate_render, **dict(render, allmap=z(6, H, W)))
    add("TSDFVolume.integrate_render 2-d", vol.integrate_render, **dict(render, allmap=z(H, W)))
    add("TSDFVolume.integrate_render device", vold.integrate_render, **{k: on(v) if isinstance(v, torch.Tensor) else v for k, v in render.items()})
    add("TSDFVolume.extract_mesh cpu", vol.extract_mesh)
    add("TSDFVolume.extract_mesh device", vold.extract_mesh)

    # ---- recon
    Vc, Tc = z(5, 3), z(4, 3, dtype=torch.int32)
    Vd, Td = on(Vc), on(Tc)
    for what, args in (("cpu", (Vc, Tc, 10)), ("vertices 4 columns", (z(5, 4), Tc, 10)), ("vertices float64", (Vc.double(), Tc, 10)),
                       ("vertices strided", (z(3, 5).t(), Tc, 10)), ("vertices empty", (z(0, 3), Tc, 10)), ("vertices numpy", (Vc.numpy(), Tc, 10)),
                       ("triangles 1-d", (Vd, on(z(4, dtype=torch.int32)), 10)), ("triangles int64", (Vd, on(z(4, 3, dtype=torch.int64)), 10)),
                       ("triangles strided", (Vd, on(z(3, 4, dtype=torch.int32).t()), 10)), ("triangles on cpu", (Vd, Tc, 10)),
                       ("n 0", (Vd, Td, 0)), ("n negative", (Vd, Td, -3)), ("n 2^28+1", (Vd, Td, (1 << 28) + 1)), ("seed negative", (Vd, Td, 10, -1)),
                       ("seed 2^32", (Vd, Td, 10, 1 << 32)), ("device", (Vd, Td, 10))):
        add(f"sample_surface {what}", recon.sample_surface, *args)
    for what, cloud in (("cpu", z(5, 3)), ("empty", z(0, 3)), ("2 columns", z(5, 2)), ("float16", z(5, 3, dtype=torch.float16)),
                        ("strided", z(3, 5).t()), ("numpy", z(5, 3).numpy())):
        add(f"PointGrid {what}", recon.PointGrid, cloud)
        add(f"cloud_metrics rec {what}", recon.cloud_metrics, cloud, z(5, 3))
        add(f"icp_align src {what}", recon.icp_align, cloud, z(5, 3))
        add(f"evaluate_reconstruction gt {what}", recon.evaluate_reconstruction, Vc, Tc, cloud)
    add("PointGrid device", recon.PointGrid, Vd)
    Q = 6
    grid = object.__new__(recon.PointGrid)  # a grid without its build
    grid.targets, grid.n, grid.device, grid.ws = Vd, 5, torch.device("cpu"), on(z(256, dtype=torch.uint8))
    q, dist, index = on(z(Q, 3)), on(z(Q)), on(z(Q, dtype=torch.int32))
    add("nearest queries on cpu", grid.nearest, z(Q, 3))
    add("nearest transform 3x3", grid.nearest, q, on(eye(3)))
    add("nearest transform float64", grid.nearest, q, on(eye(4).double()))
    add("nearest transform on cpu", grid.nearest, q, eye(4))
    add("nearest device", grid.nearest, q, on(eye(4)[:3].contiguous()))
    for what, args, kw in (("dist on cpu", (q, z(Q), index, 0.1), {}), ("dist float64", (q, on(z(Q).double()), index, 0.1), {}),
                           ("dist short", (q, on(z(Q - 1)), index, 0.1), {}), ("dist strided", (q, on(z(2 * Q)[::2]), index, 0.1), {}),
                           ("dist 2-d", (q, on(z(Q, 1)), index, 0.1), {}), ("index int64", (q, dist, on(z(Q, dtype=torch.int64)), 0.1), {}),
                           ("index on cpu", (q, dist, z(Q, dtype=torch.int32), 0.1), {}),
                           ("index dtype before dist device", (q, z(Q), on(z(Q, dtype=torch.int64)), 0.1), {}),
                           ("threshold 0", (q, dist, index, 0.0), {}), ("threshold nan", (q, dist, index, float("nan")), {}),
                           ("out short", (q, dist, index, 0.1), dict(out=on(z(17, dtype=torch.float64)))),
                           ("out float32", (q, dist, index, 0.1), dict(out=on(z(_map_lib.RECON_PAIR_DOUBLES)))),
                           ("out on cpu", (q, dist, index, 0.1), dict(out=z(_map_lib.RECON_PAIR_DOUBLES, dtype=torch.float64))),
                           ("device", (q, dist, index, 0.1), {})):
        add(f"pair_sums {what}", grid.pair_sums, *args, **kw)
    add("distance_stats 2-d", recon.distance_stats, z(4, 2), 0.1, 0.2)
    add("distance_stats cpu", recon.distance_stats, z(4), 0.1, 0.2)
    add("distance_stats float64", recon.distance_stats, on(z(4).double()), 0.1, 0.2)
    add("distance_stats out short", recon.distance_stats, dist, 0.1, 0.2, on(z(6, dtype=torch.float64)))
    add("distance_stats out on cpu", recon.distance_stats, dist, 0.1, 0.2, z(_map_lib.RECON_STATS_DOUBLES, dtype=torch.float64))
    add("distance_stats device", recon.distance_stats, dist, 0.1, 0.2)
    for thr in (0.0, -1.0, float("nan")):
        add(f"icp_align threshold {thr}", recon.icp_align, Vd, Vd, threshold=thr)
    add("icp_align init 3x3", recon.icp_align, Vd, Vd, init=torch.eye(3))
    add("icp_align max_iterations negative", recon.icp_align, Vd, Vd, max_iterations=-1)
    add("cloud_metrics distance_thresh 0", recon.cloud_metrics, Vd, Vd, distance_thresh=0.0)
    add("cloud_metrics ratio_thresh negative", recon.cloud_metrics, Vd, Vd, ratio_thresh=-1.0)
    add("cloud_metrics transform 3x3", recon.cloud_metrics, Vd, Vd, transform=on(eye(3)))
    add("cloud_metrics transform on cpu", recon.cloud_metrics, Vd, Vd, transform=eye(4))
    add("evaluate_reconstruction n_samples 0", recon.evaluate_reconstruction, Vd, Td, Vd, n_samples=0)
    add("evaluate_reconstruction icp_threshold 0", recon.evaluate_reconstruction, Vd, Td, Vd, icp_threshold=0.0)
    return cases


def refusals_block():
    """One line per case: `refuse <case>: RuntimeError: <text>`, or ACCEPTED when every check before the first library call
    passed.  Another exception type is printed as it is."""
    kept = _map_lib.call, _map_lib.lib
    _map_lib.call = _map_lib.lib = _reached
    try:
        for name, thunk in refusal_cases():
            try:
                thunk()
                line = "ACCEPTED"
            except _Reached:
                line = "ACCEPTED"
            except Exception as e:  # noqa: BLE001
                line = f"{type(e).__name__}: {e}"
            print(f"refuse {name}: " + " ".join(line.split()), flush=True)
    finally:
        _map_lib.call, _map_lib.lib = kept


def gpu_block(dev):
    w2c = rigid(23.0, [0.2, 0.9, -0.4], [0.3, -0.2, 0.8], dev)
    for W, H in ((67, 45), (131, 97)):
        allmap, gt_color, gt_depth, K = make_frame(W, H, dev, seed=W)
        for mode in ("splatam", "edge", "all"):
            for activated in (False, True):
                out = densify.seed_from_frame(allmap, gt_color, gt_depth, K, w2c, mode=mode, sil_thres=0.5, edge_thres=0.4,
                                              activated=activated)
                emit(f"seed_from_frame {mode} {W}x{H} activated={int(activated)} n={out['pixel_index'].numel()}", *out.values())
    emit("frame_stats 67x45", pose.frame_stats(*(make_frame(67, 45, dev, seed=67)[i] for i in (0, 2))))
    emit("frame_stats 67x45 no_weight_norm", pose.frame_stats(*(make_frame(67, 45, dev, seed=67)[i] for i in (0, 2)), use_weight_norm=False))

    for P in (1, 1023, 1025, 4099):
        for activated in (False, True):
            opt, _ = make_opt(P, dev, seed=P, activated=activated)
            gone = densify.prune_gaussians(opt, 0.05, 5e-4, 0.1, activated=activated)
            emit(f"prune_gaussians P={P} activated={int(activated)} removed={gone}", *map_buffers(opt))

        opt, g = make_opt(P, dev, seed=100 + P)
        stats = densify.DensificationStats(opt)
        for _ in range(3):
            radii = torch.randint(-1, 3, (P,), generator=g, dtype=torch.int32).to(dev)
            grad = (4e-4 * torch.randn(P, 3, generator=g)).to(dev)
            stats.add(radii, grad)
        emit(f"densification_stats P={P}", *stats.current())
        res = densify.densify_and_prune(opt, stats, DENSIFY, generator=torch.Generator(device=dev).manual_seed(7))
        emit(f"densify_and_prune P={P} {tuple(res)}", *map_buffers(opt), *stats.current())

    transfer = localmap.transfer_matrix(rigid(37.0, [0.3, -0.8, 0.5], [0.4, -1.1, 0.7], dev), rigid(-11.0, [0.1, 0.2, 0.9], [0.0, 0.2, -0.1], dev))
    for P, n in ((0, 5), (7, 0), (1025, 333), (4099, 1024)):
        opt, g = make_opt(P, dev, seed=200 + P)
        params = {k: v.to(dev) for k, v in make_fields(n, g).items()}
        rows = localmap.merge_local_map(opt, params, transfer, opacity_cap=0.01)
        emit(f"merge_local_map P={P} n={n} rows={rows}", *map_buffers(opt))

    for P in (1, 3, 63, 1025):
        opt, g = make_opt(P, dev, seed=300 + P, cls=mapping.RawGaussianAdam)
        for it in range(2):
            leaves = opt.render_leaves()
            emit(f"raw render_leaves P={P} step={it}", *leaves.values())
            opt.bucket.flat.copy_(1e-2 * torch.randn(13 * P, generator=g))
            raw = torch.empty(13 * P, dtype=torch.float32, device=dev)
            opt.step(leaves=leaves, raw_grad_out=raw)
            emit(f"raw step P={P} step={it}", *map_buffers(opt), raw)

    start = rigid(4.0, [0.5, -0.3, 0.8], [0.02, -0.05, 0.04], dev)
    for left in (None, rigid(61.0, [-0.7, 0.1, 0.7], [1.0, 2.0, -0.5], dev)):
        g = torch.Generator().manual_seed(400)
        opt = pose.PoseOptimizer(start, betas=(0.7, 0.99), converged_th=5e-4, left=left)
        emit(f"pose init left={int(left is not None)}", opt.w2c, *(v for v in opt.state().values() if isinstance(v, torch.Tensor)))
        for it in range(3):
            opt.step(grad=(1e-1 * torch.randn(4, 4, generator=g)).to(dev))
            st = opt.state()
            emit(f"pose step {it} left={int(left is not None)} steps={st['steps']} conv={st['converged_times']} done={st['done']}",
                 opt.w2c, *(v for v in st.values() if isinstance(v, torch.Tensor)))


def eval_tsdf_recon_block(dev):
    """The three newest parts at small, ragged sizes: 203x171 is just above the 160-pixel minimum of MS-SSIM on both sides and a
    multiple of no tile; the 20x18x17 volume sees a tilted plane through two 64x48 frames."""
    W, H = 203, 171
    allmap, gt_color, gt_depth, _ = make_frame(W, H, dev, seed=500)
    color = (gt_color.permute(2, 0, 1) + 0.2 * torch.randn(3, H, W, generator=torch.Generator().manual_seed(501)).to(dev)).contiguous()
    for clamp in (False, True):
        emit(f"frame_metrics {W}x{H} clamp_color={int(clamp)}", evaluate.frame_metrics(color, allmap, gt_color, gt_depth, clamp_color=clamp))
    ws, out = evaluate.workspace(W, H, dev), torch.zeros((2, evaluate.EVAL_OUT_DOUBLES), dtype=torch.float64, device=dev)
    evaluate.frame_metrics(color, allmap, gt_color, gt_depth, use_weight_norm=False, out=out[1], ws=ws)
    emit(f"frame_metrics {W}x{H} no_weight_norm, out row, kept ws", out)

    W, H = 64, 48
    intr = (60.0, 62.0, 31.5, 23.5)
    g = torch.Generator().manual_seed(502)
    frames = []
    for k, w2c in enumerate((rigid(3.0, [0.2, 1.0, 0.1], [0.02, -0.01, 0.03], dev), rigid(-4.0, [1.0, 0.3, -0.2], [-0.03, 0.02, -0.02], dev))):
        v, u = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        depth = 1.0 + 0.004 * (u - 32) - 0.003 * (v - 24) + 0.01 * torch.randn(H, W, generator=g)
        depth[torch.rand(H, W, generator=g) < 0.03] = 0.0
        alpha = 0.7 + 0.3 * torch.rand(H, W, generator=g)
        am = torch.randn(7, H, W, generator=g)
        am[0], am[1] = depth * alpha, alpha
        frames.append((torch.rand(3, H, W, generator=g).to(dev), depth.to(dev), am.to(dev), w2c))
    mesh = None
    for rgb8 in (True, False):
        vol = tsdf.TSDFVolume((-0.5, -0.45, 0.6), (20, 18, 17), voxel_length=0.05, sdf_trunc=0.15, depth_trunc=3.0, device=dev)
        for col, depth, _, w2c in frames:
            vol.integrate(col, depth, intr, w2c, rgb8=rgb8)
        emit(f"tsdf integrate 20x18x17 rgb8={int(rgb8)}", vol.planes)
        mesh = vol.extract_mesh()
        emit(f"tsdf extract_mesh after integrate rgb8={int(rgb8)} V={len(mesh[0])} T={len(mesh[2])}", *mesh)
        vol.reset()
        for col, _, am, w2c in frames:
            vol.integrate_render(col, am, intr, w2c, rgb8=rgb8)
        emit(f"tsdf integrate_render 20x18x17 rgb8={int(rgb8)}", vol.planes)
        emit(f"tsdf extract_mesh after integrate_render rgb8={int(rgb8)}", *vol.extract_mesh())

    vertices, _, triangles = mesh
    points, tri = recon.sample_surface(vertices, triangles, 5000, seed=3)
    emit("recon sample_surface 5000", points, tri)
    g = torch.Generator().manual_seed(503)
    targets = (torch.tensor([0.0, 0.0, 1.0]) + torch.tensor([0.5, 0.45, 0.1]) * (2.0 * torch.rand(3001, 3, generator=g) - 1.0)).to(dev)
    grid = recon.PointGrid(targets)
    move = rigid(5.0, [0.1, 0.3, 1.0], [0.03, -0.02, 0.01], dev)
    for name, m in (("no transform", None), ("transform", move)):
        dist, index = grid.nearest(points, m)
        emit(f"recon nearest 5000 -> 3001 {name}", dist, index)
        emit(f"recon pair_sums {name}", grid.pair_sums(points, dist, index, 0.05, m)[:_map_lib.RECON_PAIR_VALUES])
        emit(f"recon distance_stats {name}", recon.distance_stats(dist, 0.02, 0.05)[:_map_lib.RECON_STATS_VALUES])


def main():
    build.build()
    host_block()
    refusals_block()
    if not torch.cuda.is_available():
        print("# no GPU: the device cases were not run")
        return
    gpu_block(torch.device("cuda", 0))
    eval_tsdf_recon_block(torch.device("cuda", 0))


if __name__ == "__main__":
    main()
