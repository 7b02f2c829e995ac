"""Novel-view evaluation of a saved run: the reference's scripts/eval_nvs.py.

    python -m gaus_slam_amd.nvs RUN_DIR [--basedir D] [--lpips ALEX LIN] [--no-renders]

Loads RUN_DIR/save (scene_io.load_scene: what `python -m gaus_slam_amd.run ... --save-scene` or the reference's save_scence
wrote), opens the TEST split of the ScanNet++ sequence its `data` section names (the first train image first, as the anchor;
--basedir overrides the saved basedir), activates the raw parameters (gs2d_map_activate) and runs evaluate.evaluate_nvs into
RUN_DIR/nvs_result: psnr.txt, rmse.txt, l1.txt, ssim.txt, (lpips.txt,) nvs_result.json and, unless --no-renders,
rendering/{rgb,depth,diff}/GauS_%04d.png.  --lpips takes the two weight files of lpips.LPIPS.from_files; without it the
"LPIPS: " entry is null.  A scene of another dataset is refused with the reference's sentence and exit status 2."""
import argparse
import os
import sys

REFUSAL = "Only support NVS on ScanNet++ dataset !!!"  # scripts/eval_nvs.py:29


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m gaus_slam_amd.nvs", description=__doc__.split("\n\n")[0])
    ap.add_argument("run_dir")
    ap.add_argument("--basedir", default=None)
    ap.add_argument("--lpips", nargs=2, metavar=("ALEX", "LIN"), default=None)
    ap.add_argument("--no-renders", action="store_true")
    a = ap.parse_args(argv)
    from . import datasets, evaluate, scene_io
    config, raw, _, _ = scene_io.load_scene(os.path.join(a.run_dir, "save"), device="cpu")  # the refusal needs no device
    data = dict(config.get("data") or {})
    if str(data.get("dataset_name")).lower() != "scannetpp":
        print(REFUSAL, file=sys.stderr)
        return 2
    data["use_train_split"] = False  # eval.py:129
    data.pop("gradslam_data_cfg", None)  # ScanNet++ takes its camera from the sequence's own json
    if a.basedir is not None:
        data["basedir"] = a.basedir
    seq = datasets.open_sequence(data)
    cam = config.get("cameras") or {}
    size = datasets.working_size(data) or ((int(cam["width"]), int(cam["height"])) if "width" in cam and "height" in cam else seq.size)
    render = config.get("render") or {}
    kw = {k: render[k] for k in ("use_weight_norm", "eps", "depth_near", "depth_far") if k in render}
    model = None
    if a.lpips is not None:
        from . import lpips
        model = lpips.LPIPS.from_files(a.lpips[0], a.lpips[1])
    out = os.path.join(a.run_dir, "nvs_result")
    raw = {n: t.to("cuda") for n, t in raw.items()}
    res = evaluate.evaluate_nvs(scene_io.activate(raw), seq, size, use_sa=bool(render.get("use_sa", True)), lpips=model, out_dir=out,
                                save_renders=not a.no_renders, **kw)
    print(f"{len(seq)} views: mean PSNR {res['mean_psnr']:.2f} dB, depth RMSE {res['mean_depth_rmse'] * 100:.2f} cm, depth L1 "
          f"{res['mean_depth_l1'] * 100:.2f} cm, MS-SSIM {res['mean_ms_ssim']:.3f} -> {out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
