"""Evaluation of a saved run on every frame of its sequence: the reference's scripts/eval.py.

    python -m gaus_slam_amd.eval_final RUN_DIR [--basedir D] [--meshdir D] [--lpips ALEX LIN] [--save-renders] [--no-mesh]
                                               [--mesh-interval N] [--out DIR]

Loads RUN_DIR/save (scene_io.load_scene: what `python -m gaus_slam_amd.run ... --save-scene` or the reference's save_scence
wrote), opens the TRAIN split of the sequence its `data` section names with the run's own start / end / stride (--basedir
overrides the saved basedir), activates the raw parameters (gs2d_map_activate) and runs evaluate.evaluate_final into
RUN_DIR/eval_result, or into --out: psnr.txt, rmse.txt, l1.txt, ssim.txt, (lpips.txt,) result.json, with --save-renders
rendering/{rgb,depth}/GauS_%04d.png and rendering/diff/differ_%04d.png, and, unless --no-mesh (scripts/eval.py forces
eval_mesh), mesh/final_mesh.ply from every mesh_interval-th render (--mesh-interval, else the saved eval.mesh_interval, else 5).
The working size is the saved desired_image_width / height, else the saved cameras section, else the sequence's; the
intrinsics are the saved cameras.intrinsics where present, else the sequence's, scaled.

The mesh is scored (mesh/cleaned_mesh.ply, reconstruction_metrics.json) when the ground truth is on disk: for Replica
{meshdir}/{scene}.ply and {meshdir}/{scene}_pc_unseen.npy, meshdir from --meshdir, else the saved data.meshdir; for ScanNet++
{basedir}/{scene}/scans/mesh_aligned_0.05.ply and no unseen points.  For another dataset, or a file that is not there, the mesh
is still written and one line on stderr names what was not found.  A missing save directory and a sequence whose length differs
from the saved trajectory are refused with one line on stderr and exit status 2."""
import argparse
import os
import sys


def dataset_name(data):
    """The lower-case dataset name of a `data` section: its dataset_name, else the one its camera file gives."""
    name = data.get("dataset_name")
    if name is None and "gradslam_data_cfg" in data:
        from . import datasets
        name = datasets.load_camera(data["gradslam_data_cfg"]).get("dataset_name")
    return str(name).lower()


def ground_truth(data, meshdir=None, prog="gaus_slam_amd.eval_final"):
    """(gt_mesh, unseen) of the run a `data` section describes: (vertices, triangles) from ply.read_triangle_mesh and the
    [N,3] float32 unseen points, or (None, None) with one line on stderr that names what was not found."""
    import numpy as np
    from . import ply
    name, scene = dataset_name(data), os.path.basename(str(data.get("sequence")))
    meshdir = meshdir if meshdir is not None else data.get("meshdir")
    if name == "replica" and meshdir is not None:
        paths = [os.path.join(str(meshdir), f"{scene}.ply"), os.path.join(str(meshdir), f"{scene}_pc_unseen.npy")]
    elif name == "scannetpp":
        paths = [os.path.join(str(data.get("basedir")), scene, "scans", "mesh_aligned_0.05.ply")]
    else:
        what = "no meshdir is given (--meshdir, or data.meshdir)" if name == "replica" else f"no ground-truth mesh is known for the dataset {name!r}"
        print(f"{prog}: the mesh is not scored: {what}", file=sys.stderr)
        return None, None
    for p in paths:
        if not os.path.isfile(p):
            print(f"{prog}: the mesh is not scored: {p} was not found", file=sys.stderr)
            return None, None
    unseen = np.load(paths[1]).astype(np.float32).reshape(-1, 3) if len(paths) == 2 else None
    return ply.read_triangle_mesh(paths[0]), unseen


def summary(n, res, out):
    """The one line both commands print."""
    line = (f"{n} frames: mean PSNR {res['mean_psnr']:.2f} dB, depth RMSE {res['mean_depth_rmse'] * 100:.2f} cm, depth L1 "
            f"{res['mean_depth_l1'] * 100:.2f} cm, MS-SSIM {res['mean_ms_ssim']:.3f}, ATE RMSE {res['ate_rmse'] * 100:.2f} cm")
    rec = res.get("reconstruction")
    if rec is not None:
        l1 = rec.get("depth_l1")
        line += f", F-score {rec['fscore']:.2f}, mesh Depth L1 {'null' if l1 is None else format(l1, '.2f') + ' cm'}"
    return f"{line} -> {out}"


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m gaus_slam_amd.eval_final", description=__doc__.split("\n\n")[0])
    ap.add_argument("run_dir")
    ap.add_argument("--basedir", default=None)
    ap.add_argument("--meshdir", default=None)
    ap.add_argument("--lpips", nargs=2, metavar=("ALEX", "LIN"), default=None)
    ap.add_argument("--save-renders", action="store_true")
    ap.add_argument("--no-mesh", action="store_true")
    ap.add_argument("--mesh-interval", type=int, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    from . import datasets, evaluate, scene_io
    save = os.path.join(a.run_dir, "save")
    if not os.path.isdir(save):
        print(f"gaus_slam_amd.eval_final: {save} is no directory: run with --save-scene first", file=sys.stderr)
        return 2
    config, raw, est, gt = scene_io.load_scene(save, device="cpu")  # the refusals need no device
    data = dict(config.get("data") or {})
    data["use_train_split"] = True
    if a.basedir is not None:
        data["basedir"] = a.basedir
    if dataset_name(data) == "scannetpp":
        data.pop("gradslam_data_cfg", None)  # ScanNet++ takes its camera from the sequence's own json
    seq = datasets.open_sequence(data)
    if len(seq) != int(est.shape[0]):
        print(f"gaus_slam_amd.eval_final: the sequence holds {len(seq)} frames, the saved trajectory {int(est.shape[0])} poses", file=sys.stderr)
        return 2
    cam = config.get("cameras") or {}
    size = datasets.working_size(data) or ((int(cam["width"]), int(cam["height"])) if "width" in cam and "height" in cam else seq.size)
    render = config.get("render") or {}
    kw = {k: render[k] for k in ("use_weight_norm", "eps", "depth_near", "depth_far") if k in render}
    mesh = not a.no_mesh
    interval = a.mesh_interval if a.mesh_interval is not None else int((config.get("eval") or {}).get("mesh_interval", 5))
    gt_mesh, unseen = ground_truth(data, a.meshdir) if mesh else (None, None)
    model = None
    if a.lpips is not None:
        from . import lpips
        model = lpips.LPIPS.from_files(a.lpips[0], a.lpips[1])
    out = a.out if a.out is not None else os.path.join(a.run_dir, "eval_result")
    raw = {n: t.to("cuda") for n, t in raw.items()}
    res = evaluate.evaluate_final(scene_io.activate(raw), seq, size, est, gt, intrinsics=cam.get("intrinsics"),
                                  use_sa=bool(render.get("use_sa", True)), lpips=model, out_dir=out, save_renders=a.save_renders, mesh=mesh,
                                  mesh_interval=interval, dataset_name=dataset_name(data), gt_mesh=gt_mesh, unseen=unseen, **kw)
    print(summary(len(seq), res, out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
