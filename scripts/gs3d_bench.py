#!/usr/bin/env python
"""Times forward + backward of the 3DGS ablation renderer at 640 x 480 on the synthetic scene of gaus_slam_amd.scene_synth, at the
Gaussian counts of bench.py's `b200k` and `op` workloads (200 000 and 500 000, regime "mapping"):

  one_pass    render3d.render: ONE NC = 6 call, channels (r, g, b, z, 1, z^2) -- projected, binned, sorted and blended once
  two_pass    the structure of the reference's render_3dgs.render through the drop-in name diff_gaussian_rasterization: TWO
              NC = 3 calls over the same Gaussians, the colours and then (z, 1, z^2)
  gs2d        the 2DGS operator (gaus_slam_amd.render.render) on the same scene: it exists at the parent commit and is the
              yardstick.  It renders colour and the seven allmap channels in one call.

The scene's surfels have two scales; the 3D Gaussians get a third one, 0.05 x the mean of the two: a flat disc with the surfel's
footprint.  Every side's upstream gradient is N(0, 1) / HW on the colour, depth and silhouette channels.  The protocol is that of
scripts/benchlib.py: one process, the sides alternating, a repetition timed with the host clock around work that ends in a device
synchronise.  Nobody has measured this before: no ratio is assumed and no threshold is set; a side is faster only where the
ranges do not overlap.  Writes one JSON line to profiles/gs3d_bench.json.  Run it under a time limit, e.g.
    timeout -k 10 300 python scripts/gs3d_bench.py
"""
import argparse

import torch

import benchlib

from gaus_slam_amd import _gs3d_lib, _lib, build, render as gs_render, render3d
from gaus_slam_amd.scene_synth import make_scene

W, H = 640, 480
COUNTS = (200000, 500000)


def two_pass(cam, means3D, means2D, opacities, colors_precomp, scales, rotations):
    """render_3dgs.render's two rasterizer calls (its zero-filled dict entries are left out: they cost the same on every side)."""
    from diff_gaussian_rasterization import GaussianRasterizer as Renderer
    color_map, radius, _ = Renderer(cam)(means3D, means2D, opacities=opacities, colors_precomp=colors_precomp, scales=scales,
                                         rotations=rotations)
    w2c = cam.viewmatrix.squeeze().T
    pts4 = torch.cat((means3D, torch.ones_like(means3D[:, :1])), dim=-1)
    depth_z = (w2c @ pts4.transpose(0, 1)).transpose(0, 1)[:, 2].unsqueeze(-1)
    depth_silhouette = torch.cat((depth_z, torch.ones_like(depth_z), torch.square(depth_z)), dim=1)
    sil_map, _, _ = Renderer(cam)(means3D, means2D, opacities=opacities, colors_precomp=depth_silhouette, scales=scales,
                                  rotations=rotations)
    return {"render_color": color_map, "radius": radius, "render_depth": sil_map[0:1], "render_alpha": sil_map[1:2]}


def main():
    ap = argparse.ArgumentParser()
    benchlib.protocol_args(ap, "gs3d_bench.json")
    ap.add_argument("--gaussians", type=int, nargs="*", default=list(COUNTS))
    a = ap.parse_args()
    benchlib.need_gpu("gs3d_bench")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    up = (torch.randn((5, H, W), generator=g) / (H * W)).to(dev)  # colour, depth, silhouette
    out = dict(bench="gs3d_bench", width=W, height=H, reps=a.reps, warmup=a.warmup, device=torch.cuda.get_device_name(0),
               gs3d_source_hash=build.gs3d_source_hash(), gs3d_build_info=_gs3d_lib.build_info(), source_hash=build.source_hash(),
               build_info=_lib.build_info(), torch_version=torch.__version__, cases=[])
    for P in a.gaussians:
        sc = make_scene(P, W, H, seed=0, regime="mapping")
        cam2 = gs_render.settings_from_camera(sc["cam"], dev, use_sa=True)
        K = sc["cam"].K
        cam3 = render3d.setup_camera(W, H, K.tolist(), sc["cam"].w2c, device=dev)
        third = 0.05 * sc["scales"].mean(1, keepdim=True)
        base = {k: sc[k].to(dev) for k in ("means3D", "opacities", "rotations", "colors")}
        scales = {"gs2d": sc["scales"].to(dev), "gs3d": torch.cat((sc["scales"], third), 1).contiguous().to(dev)}

        def setup(name):
            p = {k: v.clone().requires_grad_(True) for k, v in base.items()}
            p["scales"] = scales["gs2d" if name == "gs2d" else "gs3d"].clone().requires_grad_(True)
            p["means2D"] = torch.zeros_like(p["means3D"]).requires_grad_(True)
            return p

        def run3(fn):
            def side(p):
                pkg = fn(cam3, p["means3D"], p["means2D"], p["opacities"], p["colors"], p["scales"], p["rotations"])
                image = torch.cat((pkg["render_color"], pkg["render_depth"], pkg["render_alpha"]))
                image.backward(up)
                return pkg
            return side

        def run2(p):
            pkg = gs_render.render(cam2, p["means3D"], p["means2D"], p["opacities"], colors_precomp=p["colors"], scales=p["scales"],
                                   rotations=p["rotations"])
            image = torch.cat((pkg["render_color"], pkg["allmap"][0:2]))
            image.backward(up)
            return pkg

        sides = {"one_pass": run3(render3d.render), "two_pass": run3(two_pass), "gs2d": run2}
        wall, _ = benchlib.time_sides(sides, a.reps, a.warmup, setup)
        case = dict(gaussians=P)
        for name in sides:
            case.update(benchlib.summary(wall[name], f"{name}_ms"))
        case["one_pass_over_gs2d"] = round(case["one_pass_ms_median"] / case["gs2d_ms_median"], 4)
        case["one_pass_over_two_pass"] = round(case["one_pass_ms_median"] / case["two_pass_ms_median"], 4)
        case["one_vs_two_ranges_overlap"] = benchlib.ranges_overlap(wall["one_pass"], wall["two_pass"])
        case["one_vs_gs2d_ranges_overlap"] = benchlib.ranges_overlap(wall["one_pass"], wall["gs2d"])
        from gaus_slam_amd import rasterizer3d
        case["gs3d_num_rendered"] = rasterizer3d._CAPACITY.get(dev)
        out["cases"].append(case)
    benchlib.write(out, a.out)


if __name__ == "__main__":
    main()
