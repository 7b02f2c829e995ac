"""GPU tests of evaluate.evaluate_final, the reference's eval_final over every frame of a sequence, and of the two commands that
run it.  Nothing here is compared with a number of the reference: its eval_final needs cv2, open3d, evo, pytorch_msssim and
trimesh, none of which is installed.  What is tested is that the protocol is composed as the reference writes it, from parts that
are each held to their own references elsewhere (tests/test_gpu_eval.py, test_gpu_vol.py, test_gpu_recon.py, test_gpu_mesh.py).

Bounds.  One: the mesh extrinsics against the float64 statement of tests/eval_final_ref.py, per entry
16 * 2^-23 * max(1, max|entry|)^2, the bound DESIGN.md 7.14 derives for frontend_ops.compose.  Everything else is bit equality
with existing public calls on the same inputs.

The scene is sequence.BoxRoomSequence(6, size=(224, 168)) (MS-SSIM needs a smaller side above 160) and a map seeded from its
first frame with localmap.create_map: no optimisation and no SLAM run.  The estimated trajectory is the true one with a fixed
perturbation of 2 mm and 0.1 degrees on frames 1-5, so the ATE is not zero."""
import json
import os

import numpy as np
import pytest
import torch

from tests import eval_final_ref as ref
from tests import front_ref as fr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
W, H, K = 224, 168, 6
LRS = dict(xyz=1e-4, opacity=0.05, scaling=1e-3, rotation=1e-3, rgb=2.5e-3)
G = ref.rigid(30.0, 2, (0.8, -0.4, 0.6))  # where the first camera stands in the "dataset's world" of the placement tests
FUSED = (0, 2, 4)  # k % 2 == 0
N_VIEWS = 40  # of the 2-D depth metric: the room's mesh has over a million vertices, and the default 1000 views take seconds


class Carried:
    """A sequence whose every pose is left-multiplied by the rigid G: the images are unchanged, the world is another."""

    def __init__(self, seq, G):
        self.seq, self.G = seq, torch.from_numpy(G)
        self.size, self.intrinsics, self.png_depth_scale = seq.size, seq.intrinsics, seq.png_depth_scale

    def __len__(self):
        return len(self.seq)

    def frame(self, k):
        color, depth, c2w = self.seq.frame(k)
        return color, depth, (self.G @ self.seq.pose(k)).float()

    def __iter__(self):
        return (self.frame(k) for k in range(len(self)))


def box_mesh(seq, carry):
    """The twelve triangles of the room's walls, carried by the 4x4 `carry`: (vertices float32 [8,3], triangles int32 [12,3])."""
    lo, hi = seq.box
    corners = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)], np.float64)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tri = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    v = corners @ carry[:3, :3].T + carry[:3, 3]
    return v.astype(np.float32), tri


def wall_distance(points, seq, carry):
    """The distance of every point (world of `carry`) from the nearest wall plane of the box."""
    inv = np.linalg.inv(carry)
    p = np.asarray(points, np.float64) @ inv[:3, :3].T + inv[:3, 3]
    lo, hi = (np.array(v) for v in seq.box)
    return np.minimum(np.abs(p - lo), np.abs(p - hi)).min(1)


def _render(params, settings):
    from gaus_slam_amd import render
    with torch.no_grad():
        return render.render(settings, params["means3D"], torch.zeros_like(params["means3D"]), params["opacities"],
                             colors_precomp=params["colors"], scales=params["scales"], rotations=params["rotations"])


@pytest.fixture(scope="module")
def scene():
    from gaus_slam_amd import evaluate, frontend_ops as ops, localmap, scene_io, sequence
    dev = torch.device("cuda:0")
    seq = sequence.BoxRoomSequence(K, size=(W, H))
    intr = ops.scaled_intrinsics(seq.intrinsics, seq.size, (W, H))
    frames = [ops.ingest(c.to(dev), d.view(torch.int16).to(dev), seq.png_depth_scale, (W, H)) for c, d, _ in seq]
    fx, fy, cx, cy = intr
    opt = localmap.create_map(frames[0][0], frames[0][1], torch.tensor([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]]), LRS)
    params = scene_io.activate(localmap.extract_params(opt))
    gt = np.stack([np.linalg.inv(seq.pose(k).numpy()) for k in range(K)])  # relative to the first frame, whose pose is I
    est = gt.copy()
    for k in range(1, K):  # 2 mm and 0.1 degrees, about and along an axis that changes with the frame
        shift = np.zeros(3)
        shift[k % 3] = 0.002
        est[k] = ref.rigid(0.1, k % 3, shift) @ gt[k]
    est_t, gt_t = (torch.from_numpy(m.astype(np.float32)).to(dev) for m in (est, gt))
    settings = ops.cameras(W, H, intr, est_t, use_sa=True)
    want = evaluate.evaluate_map(params, [(s, c, d) for s, (c, d) in zip(settings, frames)], est_w2cs=est_t, gt_w2cs=gt_t)
    return dict(seq=seq, intr=intr, frames=frames, params=params, est=est_t, gt=gt_t, settings=settings, want=want)


# ------------------------------------------------------------------------------------------------------------------------ metrics
def test_rows_equal_evaluate_map_over_the_same_frames(scene, tmp_path):
    from gaus_slam_amd import _front_lib, _lib, _map_lib, evaluate
    out = str(tmp_path / "final")
    res = evaluate.evaluate_final(scene["params"], scene["seq"], (W, H), scene["est"], scene["gt"], mesh=False, prefetch=0, out_dir=out)
    want = scene["want"]
    assert res["per_frame"].shape == (K, evaluate.EVAL_OUT_DOUBLES) and np.array_equal(res["per_frame"], want["per_frame"])
    for name in ("psnr", "ms_ssim", "depth_rmse", "depth_l1"):
        assert np.array_equal(res[name], want[name]) and res["mean_" + name] == want["mean_" + name], name
    assert res["ate_rmse"] == want["ate_rmse"] and 1e-4 < res["ate_rmse"] < 1e-2  # millimetres: the perturbation, not zero
    assert np.all(res["psnr"] > 15.0) and np.all(np.isfinite(res["per_frame"]))
    assert "mesh" not in res and "mesh_extrinsics" not in res and "reconstruction" not in res and "lpips" not in res
    ahead = evaluate.evaluate_final(scene["params"], scene["seq"], (W, H), scene["est"], scene["gt"], prefetch=2)
    assert ahead["per_frame"].tobytes() == res["per_frame"].tobytes() and ahead["result"] == res["result"]
    assert sorted(os.listdir(out)) == ["l1.txt", "psnr.txt", "result.json", "rmse.txt", "ssim.txt"]
    for name, key in (("psnr.txt", "psnr"), ("rmse.txt", "depth_rmse"), ("l1.txt", "depth_l1"), ("ssim.txt", "ms_ssim")):
        rows = np.loadtxt(os.path.join(out, name))
        assert rows.shape == (K,) and np.array_equal(rows, res[key]), name
    result = json.load(open(os.path.join(out, "result.json")))
    assert list(result) == list(evaluate.FINAL_KEYS) + ["build"] and result == res["result"]
    assert result["LPIPS: "] is None and result["PSNR: "] == res["mean_psnr"] and result["SSIM: "] == res["mean_ms_ssim"]
    assert result["Depth RMSE: "] == res["mean_depth_rmse"] and result["Depth L1: "] == res["mean_depth_l1"] and result["ATE RMSE: "] == res["ate_rmse"]
    assert result["build"] == dict(rasterizer=_lib.build_info(), map=_map_lib.build_info(), front=_front_lib.build_info())


def test_lpips_rows_and_saved_renders(scene, tmp_path):
    """With a model the second row tensor and lpips.txt; with save_renders the three PNG names of evaluate_map(dump_dir=...),
    with its bytes."""
    from PIL import Image
    from gaus_slam_amd import evaluate, lpips
    model = lpips.LPIPS.random(3)
    frames = [(s, c, d) for s, (c, d) in zip(scene["settings"], scene["frames"])]
    want_dir, out = str(tmp_path / "map"), str(tmp_path / "final")
    want = evaluate.evaluate_map(scene["params"], frames, lpips=model, dump_dir=want_dir)
    res = evaluate.evaluate_final(scene["params"], scene["seq"], (W, H), scene["est"], scene["gt"], lpips=model, out_dir=out, save_renders=True)
    assert np.array_equal(res["per_frame"], scene["want"]["per_frame"])
    assert np.array_equal(res["lpips_per_frame"], want["lpips_per_frame"]) and res["mean_lpips"] == want["mean_lpips"] == res["result"]["LPIPS: "]
    assert np.loadtxt(os.path.join(out, "lpips.txt")).shape == (K,) and set(res["result"]["build"]) == {"rasterizer", "map", "front", "view", "lpips"}
    for sub, name in (("rgb", "GauS_%04d.png"), ("depth", "GauS_%04d.png"), ("diff", "differ_%04d.png")):
        assert sorted(os.listdir(os.path.join(out, "rendering", sub))) == [name % k for k in range(K)]
        for k in (0, K - 1):
            a, b = (np.asarray(Image.open(os.path.join(d, "rendering", sub, name % k))) for d in (out, want_dir))
            assert a.shape == (H, W, 3) and np.array_equal(a, b), (sub, k)
    with pytest.raises(RuntimeError, match="save_renders needs out_dir"):
        evaluate.evaluate_final(scene["params"], scene["seq"], (W, H), scene["est"], scene["gt"], save_renders=True)


# ---------------------------------------------------------------------------------------------------------------------- placement
NAMES = ["replica", "scannetpp"]


@pytest.fixture(scope="module")
def placed_runs(scene, tmp_path_factory):
    """evaluate_final with the mesh on the G-carried sequence, once per dataset name.  The mesh stands in the frame
    inv(P) . (the dataset's world): the ground truth is the box carried by inv(P) @ G, which is G itself unless the dataset is
    ScanNet++."""
    from gaus_slam_amd import evaluate, tsdf_blocks
    runs = {}
    for name in NAMES:
        carry = np.linalg.inv(ref.swap(name)) @ G
        gt_mesh = box_mesh(scene["seq"], carry)
        out = str(tmp_path_factory.mktemp(name) / "final")
        fused, real = [], tsdf_blocks.BlockTSDFVolume.integrate_render

        def spy(self, color, allmap, intrinsics, w2c, **kw):
            fused.append((w2c.clone(), intrinsics, kw))
            return real(self, color, allmap, intrinsics, w2c, **kw)

        tsdf_blocks.BlockTSDFVolume.integrate_render = spy
        try:
            res = evaluate.evaluate_final(scene["params"], Carried(scene["seq"], G), (W, H), scene["est"], scene["gt"], mesh=True,
                                          mesh_interval=2, dataset_name=name, gt_mesh=gt_mesh, out_dir=out, seed=4, n_views=N_VIEWS)
        finally:
            tsdf_blocks.BlockTSDFVolume.integrate_render = real
        runs[name] = dict(name=name, carry=carry, gt_mesh=gt_mesh, out=out, res=res, fused=fused)
    return runs


@pytest.fixture(params=NAMES)
def placed(request, placed_runs):
    return placed_runs[request.param]


def test_mesh_extrinsics_against_float64(scene, placed):
    E = placed["res"]["mesh_extrinsics"]
    assert tuple(E.shape) == (K, 4, 4) and E.dtype == torch.float32 and E.is_cuda
    est = scene["est"].double().cpu().numpy()
    c2w_0 = G.astype(np.float32).astype(np.float64)  # the first pose as the sequence hands it over, in float32
    want = ref.mesh_extrinsics(est, c2w_0, placed["name"])
    bound = ref.compose_bound(est, c2w_0, want)
    err = np.abs(E.double().cpu().numpy() - want).max()
    print(f"{placed['name']}: mesh extrinsics max |err| {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    swapped = np.abs(want - ref.mesh_extrinsics(est, c2w_0, "replica")).max() > 0.1
    assert swapped == (placed["name"] == "scannetpp")
    assert np.array_equal(placed["res"]["per_frame"], scene["want"]["per_frame"])  # the mesh changes no metric


def test_fused_frames_and_vertices(scene, placed):
    """Frames 0, 2 and 4 and no others, with uint8 colour; the vertices are those of the test's own volume over the same renders
    and extrinsics, moved by the float32 compensate_vector; the written file reads back equal."""
    from gaus_slam_amd import ply, tsdf_blocks
    res, E = placed["res"], placed["res"]["mesh_extrinsics"]
    assert len(placed["fused"]) == len(FUSED)
    for k, (w2c, intrinsics, kw) in zip(FUSED, placed["fused"]):
        assert torch.equal(w2c, E[k]) and tuple(intrinsics) == tuple(scene["intr"]) and kw["rgb8"] is True
    vol = tsdf_blocks.BlockTSDFVolume()
    assert (vol.voxel_length, vol.sdf_trunc, vol.depth_trunc) == (5.0 / 512.0, 0.04, 30.0)
    for k in FUSED:
        pkg = _render(scene["params"], scene["settings"][k])
        vol.integrate_render(pkg["render_color"], pkg["allmap"], scene["intr"], E[k])
    v, c, t = vol.extract_mesh()
    v = v + torch.tensor(ref.COMPENSATE_VECTOR, dtype=torch.float32, device=v.device)
    got_v, got_c, got_t = res["mesh"]
    assert v.shape[0] > 1000 and t.shape[0] > 1000
    assert torch.equal(got_v, v) and torch.equal(got_c, c) and torch.equal(got_t, t)
    file_v, file_t = ply.read_triangle_mesh(os.path.join(placed["out"], "mesh", "final_mesh.ply"))
    assert np.array_equal(file_v, got_v.cpu().numpy()) and np.array_equal(file_t, got_t.cpu().numpy())
    dist = wall_distance(file_v, scene["seq"], placed["carry"])
    print(f"{placed['name']}: {len(file_v)} vertices, median distance from the box's walls {np.median(dist) * 1000:.2f} mm, max {dist.max() * 1000:.1f} mm")


# ------------------------------------------------------------------------------------------------------------------------ scoring
def test_reconstruction_equals_the_direct_calls(scene, placed):
    from gaus_slam_amd import meshrender, ply, recon
    res, out, name = placed["res"], placed["out"], placed["name"]
    rec = res["reconstruction"]
    file_v, _, file_t = ply.read_mesh(os.path.join(out, "mesh", "final_mesh.ply"))
    v, _, t = meshrender.clean_mesh(torch.from_numpy(file_v).cuda(), None, torch.from_numpy(file_t).cuda())
    clean_v, clean_t = ply.read_triangle_mesh(os.path.join(out, "mesh", "cleaned_mesh.ply"))
    assert np.array_equal(clean_v, v.cpu().numpy()) and np.array_equal(clean_t, t.cpu().numpy())
    gt_v, gt_t = (torch.from_numpy(a).cuda() for a in placed["gt_mesh"])
    if name == "scannetpp":
        want = recon.evaluate_reconstruction(v, t, gt_v, gt_t, seed=4)
        assert rec["depth_l1"] is None and "views_used" not in rec
        want["depth_l1"] = None
    else:
        want = meshrender.evaluate_mesh(v, None, t, gt_v, gt_t, clean=False, seed=4, n_views=N_VIEWS)
        assert 1 <= rec["views_used"] <= N_VIEWS and np.isfinite(rec["depth_l1"])
    assert set(rec) == set(want)
    for key in want:
        if key == "transform":
            assert np.array_equal(rec[key], want[key]) and np.isfinite(rec[key]).all()
        else:
            assert rec[key] == want[key], key
            assert rec[key] is None and key == "depth_l1" or np.isfinite(rec[key]), key
    for key in ("accuracy", "completion", "completion_ratio", "precision", "recall", "fscore"):
        assert key in rec
    print(f"{name}: F-score {rec['fscore']:.3f}, precision {rec['precision']:.3f}, recall {rec['recall']:.3f}, accuracy {rec['accuracy']:.4f}, "
          f"completion {rec['completion']:.4f}, ICP fitness {rec['icp_fitness']:.3f}, Depth L1 {rec['depth_l1']}")
    saved = json.load(open(os.path.join(out, "reconstruction_metrics.json")))
    assert set(saved) == set(rec)
    for key in rec:
        assert saved[key] == (np.asarray(rec[key]).tolist() if key == "transform" else rec[key]), key
    assert set(res["result"]["build"]) == {"rasterizer", "map", "front", "vol", "mesh"}


def test_unseen_points_turn_the_depth_metric_on_for_scannetpp(scene, placed_runs):
    """`unseen` given: evaluate_mesh scores a ScanNet++ mesh too.  The point stands far outside the box, where no view sees it."""
    from gaus_slam_amd import evaluate
    placed = placed_runs["scannetpp"]
    res = evaluate.evaluate_final(scene["params"], Carried(scene["seq"], G), (W, H), scene["est"], scene["gt"], mesh=True, mesh_interval=2,
                                  dataset_name="ScanNetPP", gt_mesh=placed["gt_mesh"], unseen=np.array([[1e4, 1e4, -1e4]], np.float32), seed=4, n_views=N_VIEWS)
    assert torch.equal(res["mesh"][0], placed["res"]["mesh"][0])  # the dataset's name is compared without its case
    assert np.isfinite(res["reconstruction"]["depth_l1"]) and res["reconstruction"]["fscore"] == placed["res"]["reconstruction"]["fscore"]


# ------------------------------------------------------------------------------------------------------------------------ refusals
def test_a_trajectory_of_another_length_is_refused_before_the_first_render(scene, tmp_path, monkeypatch):
    from gaus_slam_amd import evaluate, render
    calls = []
    monkeypatch.setattr(render, "render", lambda *a, **k: calls.append(1))
    out = tmp_path / "final"
    with pytest.raises(RuntimeError, match="6 frames.*5 poses"):
        evaluate.evaluate_final(scene["params"], scene["seq"], (W, H), scene["est"][:5], scene["gt"][:5], out_dir=str(out), mesh=True)
    assert not calls and not out.exists()


def test_a_first_pose_that_is_not_finite_is_refused(scene):
    from gaus_slam_amd import evaluate
    bad = G.copy()
    bad[0, 3] = np.nan
    with pytest.raises(RuntimeError, match="first pose is not finite"):
        evaluate.evaluate_final(scene["params"], Carried(scene["seq"], bad), (W, H), scene["est"], scene["gt"], mesh=True)


# -------------------------------------------------------------------------------------------------------------------- command line
def test_the_two_commands_on_the_recorded_kitchen_frames(tmp_path, capsys, monkeypatch):
    """python -m gaus_slam_amd.run ... --save-scene --eval-final, then python -m gaus_slam_amd.eval_final on what it saved: the
    same map at the same poses through the same calls, so the two evaluations agree exactly.  results.json is what the runner
    writes without the flag: SlamResult.save of the very run, called again here as the runner calls it, writes the same content.
    (Two runs are not compared: run_slam itself is not bit-reproducible from run to run -- measured on an MI355X, two runs of
    these four frames ended with 63071 and 63074 Gaussians -- which has nothing to do with the flag.  That the runner without the
    flag writes its four files and nothing else is tests/test_gpu_datasets.py's.)"""
    from gaus_slam_amd import eval_final, evaluate, run, slam
    cfg = fr.slam_config(180, 320, num_tracking_iters=8, num_mapping_iters=6, num_ba_iters=2, final_refinement=2)
    del cfg["cameras"]["height"], cfg["cameras"]["width"]  # the runner takes them from the data section
    cfg["data"] = dict(dataset_name="Replica", basedir=GOLDEN, gradslam_data_cfg=os.path.join(GOLDEN, "kitchen", "camera.yaml"), sequence="kitchen",
                       desired_image_height=320, desired_image_width=180, start=0, end=-1, stride=1)
    path, d, plain = tmp_path / "kitchen.py", tmp_path / "out", tmp_path / "plain"
    path.write_text(f"config = {cfg!r}\n")
    runs, real = [], slam.run_slam
    monkeypatch.setattr(slam, "run_slam", lambda *a, **k: runs.append(real(*a, **k)) or runs[-1])
    assert run.main([str(path), "--frames", "4", "--save-scene", "--eval-final", "--out", str(d)]) == 0
    assert sorted(os.listdir(d)) == ["final_refine_result", "map.ply", "results.json", "save", "traj_est.txt", "traj_gt.txt"]
    written = json.load(open(d / "results.json"))
    runs[0].save(str(plain), data=written["data"], seed=written["seed"])  # run.main's own call, after the evaluation
    assert written["data"]["end"] == 4 and json.load(open(plain / "results.json")) == written
    for name in ("traj_est.txt", "traj_gt.txt", "map.ply"):
        assert open(plain / name, "rb").read() == open(d / name, "rb").read(), name
    assert sorted(os.listdir(d / "final_refine_result")) == ["l1.txt", "psnr.txt", "result.json", "rmse.txt", "ssim.txt"]  # no `eval` section
    assert eval_final.main([str(d), "--no-mesh"]) == 0
    printed = capsys.readouterr().out
    assert printed.count("4 frames: mean PSNR") == 2 and str(d / "eval_result") in printed
    first, second = (json.load(open(d / sub / "result.json")) for sub in ("final_refine_result", "eval_result"))
    for result in (first, second):
        assert list(result) == list(evaluate.FINAL_KEYS) + ["build"] and result["LPIPS: "] is None
        assert all(np.isfinite(result[key]) for key in evaluate.FINAL_KEYS if key != "LPIPS: ")
    assert {k: first[k] for k in evaluate.FINAL_KEYS} == {k: second[k] for k in evaluate.FINAL_KEYS}
    for name in ("psnr.txt", "rmse.txt", "l1.txt", "ssim.txt"):
        a, b = (np.loadtxt(d / sub / name) for sub in ("final_refine_result", "eval_result"))
        assert a.shape == (4,) and np.array_equal(a, b), name
    # the mesh is on by default; no ground truth is on disk for the fixture, which one line on stderr says
    assert eval_final.main([str(d), "--mesh-interval", "2", "--out", str(tmp_path / "meshed")]) == 0
    said = [line for line in capsys.readouterr().err.splitlines() if line.startswith("gaus_slam_amd.eval_final:")]
    assert len(said) == 1 and "not scored" in said[0] and "meshdir" in said[0]
    assert sorted(os.listdir(tmp_path / "meshed")) == ["l1.txt", "mesh", "psnr.txt", "result.json", "rmse.txt", "ssim.txt"]
    assert os.listdir(tmp_path / "meshed" / "mesh") == ["final_mesh.ply"]
    assert {k: json.load(open(tmp_path / "meshed" / "result.json"))[k] for k in evaluate.FINAL_KEYS} == {k: second[k] for k in evaluate.FINAL_KEYS}
