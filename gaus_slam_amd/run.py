"""The runner: a reference-format configuration file in, the results of one SLAM run out.

    python -m gaus_slam_amd.run CONFIG.py [--frames N] [--out DIR] [--seed S] [--save-scene] [--eval-final]

CONFIG.py is a Python file that defines `config` (configs/*/config*.py of the reference), loaded with runpy.  Its `data` section
names the recorded sequence (datasets.open_sequence: gradslam_data_cfg, basedir, sequence, start, end, stride, ignore_bad;
desired_image_height / desired_image_width become config['cameras']['height'] / ['width']); the other sections are the driver's
(slam.check_config lists what is read and refuses, by name, what is not wired: such a refusal is reported and the exit status is
2).  --frames N keeps the first N frames of the selection.  The run is slam.run_slam, then SlamResult.evaluate() and
SlamResult.save(DIR): results.json, traj_est.txt, traj_gt.txt and map.ply -- the loop and the tail of the reference's
scripts/gaus.py without wandb and without the Open3D windows.  DIR defaults to config['workdir'] / config['run_name'] where the
file names both, else to ./output.  --save-scene also writes DIR/save, the reference's saved scene (scene_io.save_scene: the
configuration as run, the raw map and both trajectories), which python -m gaus_slam_amd.nvs evaluates later; without the flag
the four files above are all that is written.  --eval-final then re-reads the sequence and scores EVERY frame at its estimated
pose (SlamResult.evaluate_final, the reference's eval_final) into DIR/final_refine_result, the directory scripts/gaus.py uses:
result.json is the reference's protocol, results.json the score of the frames the maps were optimised on.  The configuration's
`eval` section (eval_mesh, save_renders, mesh_interval) says whether a mesh is fused and the renders are saved; without one there
is no mesh, there are no renders and the interval is 5.  The ground-truth mesh is looked for as python -m gaus_slam_amd.eval_final
does."""
import argparse
import copy
import os
import runpy
import sys


def load_config(path):
    """The `config` dict of a reference-format configuration file."""
    scope = runpy.run_path(str(path))
    if not isinstance(scope.get("config"), dict):
        raise ValueError(f"{path} defines no dict named `config`")
    return scope["config"]


def prepare(config, frames=None):
    """(sequence, config for run_slam) of a loaded configuration: opens config['data'], hands the desired image size to
    config['cameras'] and, with `frames`, keeps the first `frames` frames of the selection."""
    from . import datasets
    if not isinstance(config.get("data"), dict):
        raise ValueError("the configuration lacks the section 'data'")
    data = dict(config["data"])
    if frames is not None:
        if int(frames) < 1:
            raise ValueError(f"--frames must be >= 1, got {frames}")
        start, stride = int(data.get("start", 0)), int(data.get("stride", 1) or 1)
        end = start + int(frames) * stride
        data["end"] = end if int(data.get("end", -1)) == -1 else min(end, int(data["end"]))
    seq = datasets.open_sequence(data)
    config = copy.deepcopy(config)
    config["data"] = data
    size = datasets.working_size(data)
    if size is not None:
        cam = config.setdefault("cameras", {})
        cam["width"], cam["height"] = size
    return seq, config


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m gaus_slam_amd.run", description=__doc__.split("\n\n")[0])
    ap.add_argument("config")
    ap.add_argument("--frames", type=int, default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--save-scene", action="store_true")
    ap.add_argument("--eval-final", action="store_true")
    a = ap.parse_args(argv)
    config = load_config(a.config)
    seed = a.seed if a.seed is not None else int(config.get("seed", 0))
    seq, config = prepare(config, a.frames)
    out = a.out
    if out is None:
        out = os.path.join(str(config["workdir"]), str(config["run_name"])) if "workdir" in config and "run_name" in config else "output"
    from . import slam
    try:
        # what run_slam fills in from the sequence is not missing
        slam.check_config({**config, "cameras": {"intrinsics": None, "width": seq.size[0], "height": seq.size[1], **config.get("cameras", {})}})
    except RuntimeError as e:
        print(f"gaus_slam_amd.run: {a.config} is refused: {e}", file=sys.stderr)
        return 2
    result = slam.run_slam(seq, config, seed=seed)
    m = result.save(out, data=config["data"], seed=seed)
    if a.save_scene:
        result.save_scene(os.path.join(out, "save"), config)
    print(f"{len(seq)} frames, {len(result.records)} local maps, {result.backend.map.soa.P} Gaussians: mean PSNR {m['mean_psnr']:.2f} dB, "
          f"mean depth L1 {m['mean_depth_l1']:.5f} m, ATE RMSE {m['ate_rmse']:.5f} m -> {out}")
    if a.eval_final:
        from . import eval_final
        ev, data = config.get("eval") or {}, config["data"]
        mesh = bool(ev.get("eval_mesh", False))
        gt_mesh, unseen = eval_final.ground_truth(data, prog="gaus_slam_amd.run") if mesh else (None, None)
        final = os.path.join(out, "final_refine_result")
        res = result.evaluate_final(seq, out_dir=final, mesh=mesh, save_renders=bool(ev.get("save_renders", False)),
                                    mesh_interval=int(ev.get("mesh_interval", 5)), dataset_name=eval_final.dataset_name(data),
                                    gt_mesh=gt_mesh, unseen=unseen)
        print(eval_final.summary(len(seq), res, final))
    return 0


if __name__ == "__main__":
    sys.exit(main())
