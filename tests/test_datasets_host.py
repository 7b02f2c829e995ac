"""CPU tests of the recorded-sequence readers (gaus_slam_amd/datasets.py), of the runner's configuration loading
(gaus_slam_amd/run.py), of the writers behind SlamResult.save and of the recorded fixture tests/golden/kitchen (the first eleven
frames of the sample sequence the reference ships: 360 x 640, JPEG colour, 16-bit PNG depth at 6553.5 units per metre, traj.txt,
camera.yaml).  Nothing here launches a kernel."""
import json
import os

import numpy as np
import pytest
import torch

from gaus_slam_amd import datasets, ply, run, slam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CAMERA = dict(image_height=5, image_width=7, fx=6.0, fy=6.5, cx=3.0, cy=2.0, png_depth_scale=1000.0, crop_edge=3)


def _write_color(path, value, size=(7, 5)):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(np.full((size[1], size[0], 3), value, np.uint8)).save(path, quality=100)


def _write_depth(path, value, size=(7, 5)):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(np.full((size[1], size[0]), value, np.uint16)).save(path)


# ----------------------------------------------------------------------------------------------------------------------- fixture
def kitchen(**kw):
    cam = datasets.load_camera(os.path.join(GOLDEN, "kitchen", "camera.yaml"))
    return datasets.ReplicaSequence(GOLDEN, "kitchen", cam["camera_params"], **kw), cam


def test_kitchen_fixture_loads_as_the_camera_file_says():
    seq, cam = kitchen()
    assert cam["dataset_name"] == "replica" and len(seq) == 11
    assert seq.size == (360, 640) and seq.depth_size == (360, 640) and seq.distortion is None and seq.crop_edge == 0
    assert seq.intrinsics == (340.3754036086746, 338.1963970958536, 180.0, 320.0) and seq.png_depth_scale == 6553.5
    frames = list(seq)
    assert len(frames) == 11
    for color, depth, c2w in frames:
        assert color.dtype == torch.uint8 and tuple(color.shape) == (640, 360, 3) and color.is_contiguous()
        assert depth.dtype == torch.uint16 and tuple(depth.shape) == (640, 360) and depth.is_contiguous()
        assert c2w.dtype == torch.float32 and tuple(c2w.shape) == (4, 4) and torch.equal(c2w[3], torch.tensor([0.0, 0.0, 0.0, 1.0]))
        R = c2w[:3, :3].double()
        assert (R @ R.T - torch.eye(3, dtype=torch.float64)).abs().max() < 1e-5  # float32 rigid poses
    assert [os.path.basename(p) for p in seq.color_paths] == [f"frame_{k:04d}.jpg" for k in range(11)]
    assert [os.path.basename(p) for p in seq.depth_paths] == [f"depth_{k:04d}.png" for k in range(11)]
    assert frames[0][0].float().std() > 20 and int(frames[0][1].to(torch.int32).max()) > 3276  # a picture, and more than half a metre deep


def _median_depth_error(depth0, depth_k, T_k_from_0, intr, scale):
    """Back-projects depth0, carries the points by T_k_from_0 (camera 0 -> camera k), projects them with `intr` and returns the
    median |z - depth_k| over the points that land on a pixel with a measurement."""
    fx, fy, cx, cy = intr
    H, W = depth0.shape
    z = depth0.astype(np.float64) / scale
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    ok = z > 0
    p = np.stack(((x - cx) / fx * z, (y - cy) / fy * z, z, np.ones_like(z)), -1)[ok] @ T_k_from_0.T
    front = p[:, 2] > 1e-6
    p = p[front]
    u, v = np.rint(p[:, 0] / p[:, 2] * fx + cx).astype(np.int64), np.rint(p[:, 1] / p[:, 2] * fy + cy).astype(np.int64)
    inside = (u >= 0) & (u < W) & (v >= 0) & (v < H)
    zk = depth_k.astype(np.float64)[v[inside], u[inside]] / scale
    seen = zk > 0
    assert seen.sum() > 0.2 * H * W  # the views overlap
    return float(np.median(np.abs(p[inside][seen, 2] - zk[seen])))


def test_kitchen_poses_intrinsics_and_depth_scale_are_consistent():
    """Frame 0's depth carried into frames 1, 5 and 10: the camera-to-world reading of traj.txt explains the depth images to a
    few millimetres, the inverse reading and no motion at all do not."""
    seq, _ = kitchen()
    frames = list(seq)
    d0 = frames[0][1].numpy()
    c2w = [f[2].double().numpy() for f in frames]
    for k in (1, 5, 10):
        dk = frames[k][1].numpy()
        args = (seq.intrinsics, seq.png_depth_scale)
        right = _median_depth_error(d0, dk, np.linalg.inv(c2w[k]) @ c2w[0], *args)
        inverse = _median_depth_error(d0, dk, c2w[k] @ np.linalg.inv(c2w[0]), *args)
        still = _median_depth_error(d0, dk, np.eye(4), *args)
        print(f"frame {k}: median |z - depth| {1e3 * right:.1f} mm as camera-to-world, {1e3 * inverse:.1f} mm as world-to-camera, "
              f"{1e3 * still:.1f} mm without motion")
        assert right < inverse and right < still and right < 0.01


# ----------------------------------------------------------------------------------------------------------------------- replica
@pytest.fixture()
def replica_dir(tmp_path):
    """Twelve frames named frame_1 .. frame_12 (no zero padding): colour k is all 10 + k, depth all 100 + k, pose k has tx = k."""
    for k in range(1, 13):
        _write_color(str(tmp_path / "room" / "results" / f"frame_{k}.jpg"), 10 + k)
        _write_depth(str(tmp_path / "room" / "results" / f"depth_{k}.png"), 100 + k)
    with open(tmp_path / "room" / "traj.txt", "w") as fh:
        for k in range(1, 15):  # more poses than frames, as in the fixture
            m = np.eye(4)
            m[0, 3] = k
            fh.write(" ".join(f"{v:.18e}" for v in m.reshape(-1)) + "\n")
    return tmp_path


def _ids(seq):
    return [(int(c[0, 0, 0]) - 10, int(d[0, 0]) - 100, int(p[0, 3])) for c, d, p in seq]


def test_replica_reader_orders_naturally_and_selects(replica_dir):
    seq = datasets.ReplicaSequence(str(replica_dir), "room", CAMERA)
    assert [os.path.basename(p) for p in seq.color_paths] == [f"frame_{k}.jpg" for k in range(1, 13)]  # frame_2 before frame_10
    assert _ids(seq) == [(k, k, k) for k in range(1, 13)]
    assert seq.size == (7, 5) and seq.depth_size == (7, 5) and seq.intrinsics == (6.0, 6.5, 3.0, 2.0) and seq.crop_edge == 3
    assert datasets.natural_key("frame_2.jpg") < datasets.natural_key("frame_10.jpg") and "frame_10.jpg" < "frame_2.jpg"
    for kw, want in ((dict(start=3), list(range(4, 13))), (dict(end=5), [1, 2, 3, 4, 5]), (dict(start=2, end=9, stride=3), [3, 6, 9]),
                     (dict(stride=5), [1, 6, 11]), (dict(stride=None), list(range(1, 13))), (dict(start=11, end=-1), [12])):
        seq = datasets.ReplicaSequence(str(replica_dir), "room", {"camera_params": CAMERA}, **kw)
        assert [i for i, _, _ in _ids(seq)] == want and _ids(seq) == [(k, k, k) for k in want], kw
        assert seq.retained == [k - 1 for k in want] and len(seq) == len(want)


def test_replica_reader_refuses(replica_dir):
    new = lambda **kw: datasets.ReplicaSequence(str(replica_dir), "room", CAMERA, **kw)
    for kw, text in ((dict(start=-1), "start"), (dict(start=4, end=4), "end"), (dict(start=4, end=2), "end"), (dict(end=0), "end"),
                     (dict(end=-2), "end"), (dict(stride=0), "stride"), (dict(start=12), "no frame")):
        with pytest.raises(ValueError, match=text):
            new(**kw)
    with pytest.raises(ValueError, match="fx"):
        datasets.ReplicaSequence(str(replica_dir), "room", {k: v for k, v in CAMERA.items() if k != "fx"})
    os.remove(replica_dir / "room" / "results" / "depth_7.png")
    with pytest.raises(ValueError, match="must be the same"):
        new()
    _write_depth(str(replica_dir / "room" / "results" / "depth_7.png"), 107, size=(6, 5))
    with pytest.raises(ValueError, match="depth_7.png is 6 x 5"):
        list(new())
    with pytest.raises(ValueError, match="the camera says 9 x 5"):
        list(datasets.ReplicaSequence(str(replica_dir), "room", {**CAMERA, "image_width": 9}))
    with pytest.raises(RuntimeError, match="Nonesuch"):
        datasets._need("nonesuch_module", "Nonesuch")


# --------------------------------------------------------------------------------------------------------------------------- TUM
TUM_COLOR = [0.00, 0.02, 0.05, 0.10, 0.50, 1.00, 1.04]
TUM_DEPTH = [0.01, 0.06, 0.11, 0.30, 1.01, 1.05]
TUM_POSE = [0.00, 0.03, 0.06, 0.09, 0.50, 1.10]
# colour 0: depth 0, pose 0.  colour 1 (0.02): depth 0, pose 1, but only 0.02 s after the kept colour 0: thinned (1/32 = 0.03125).
# colour 2 (0.05): depth 1, pose 2.  colour 3 (0.10): depth 2, pose 3.  colour 4 (0.50): the nearest depth (0.30) is 0.2 s away:
# dropped.  colour 5 (1.00): the nearest pose (1.10) is 0.10 s away: dropped.  colour 6 (1.04): depth 5 (1.05), pose 5 (1.10, 0.06 s).
TUM_WANT = [(0, 0, 0), (2, 1, 2), (3, 2, 3), (6, 5, 5)]


@pytest.fixture()
def tum_dir(tmp_path):
    rng = np.random.default_rng(0)
    quats = rng.normal(size=(len(TUM_POSE), 4)) * 1.7  # not normalised
    folder = tmp_path / "desk"
    for i, t in enumerate(TUM_COLOR):
        _write_color(str(folder / "rgb" / f"{t:.2f}.jpg"), 10 + i)
    for j, t in enumerate(TUM_DEPTH):
        _write_depth(str(folder / "depth" / f"{t:.2f}.png"), 100 + j)
    with open(folder / "rgb.txt", "w") as fh:
        fh.write("# color images\n# timestamp filename\n\n" + "".join(f"{t:.2f} rgb/{t:.2f}.jpg\n" for t in TUM_COLOR))
    with open(folder / "depth.txt", "w") as fh:
        fh.write("# depth maps\n" + "".join(f"{t:.2f} depth/{t:.2f}.png\n" for t in TUM_DEPTH))
    with open(folder / "groundtruth.txt", "w") as fh:
        fh.write("# ground truth trajectory\n# timestamp tx ty tz qx qy qz qw\n")
        for k, (t, q) in enumerate(zip(TUM_POSE, quats)):
            fh.write(f"{t:.2f} {k}.5 {-k} 0.25 " + " ".join(repr(float(v)) for v in q) + "\n")
    return tmp_path, quats


def test_tum_reader_associates_and_thins(tum_dir):
    from scipy.spatial.transform import Rotation
    root, quats = tum_dir
    cam = {**CAMERA, "distortion": [0.2624, -0.9531, -0.0054, 0.0026, 1.1633]}
    seq = datasets.TUMSequence(str(root), "desk", cam)
    assert seq.associations == TUM_WANT == datasets.associate(TUM_COLOR, TUM_DEPTH, TUM_POSE)
    assert seq.distortion == (0.2624, -0.9531, -0.0054, 0.0026, 1.1633) and seq.depth_size == (7, 5) and len(seq) == 4
    for (color, depth, c2w), (i, j, k) in zip(seq, TUM_WANT):
        assert int(color[2, 3, 1]) == 10 + i and int(depth[2, 3]) == 100 + j
        want = np.eye(4)
        want[:3, :3] = Rotation.from_quat(quats[k]).as_matrix()  # (x, y, z, w), normalised by scipy
        want[:3, 3] = (k + 0.5, -k, 0.25)
        assert np.abs(c2w.numpy() - want).max() < 1e-6 and np.abs(datasets.quaternion_pose([k + 0.5, -k, 0.25, *quats[k]]) - want).max() < 1e-14
    assert datasets.TUMSequence(str(root), "desk", {**CAMERA, "distortion": [0.1, 0.2, 0.3, 0.4]}).distortion == (0.1, 0.2, 0.3, 0.4, 0.0)
    # the bounds are strict: exactly max_dt away is not associated, exactly 1 / frame_rate later is not kept
    assert datasets.associate([0.0, 1.0], [0.5, 1.0], [0.0, 1.0], max_dt=0.5) == [(1, 1, 1)]
    assert datasets.associate([0.0, 0.25, 0.5], [0.0, 0.25, 0.5], [0.0, 0.25, 0.5], frame_rate=4) == [(0, 0, 0), (2, 2, 2)]
    sub = datasets.TUMSequence(str(root), "desk", cam, start=1, end=4, stride=2)  # the selection applies after the association
    assert [int(c[0, 0, 0]) - 10 for c, _, _ in sub] == [2, 6]
    os.rename(root / "desk" / "groundtruth.txt", root / "desk" / "pose.txt")
    assert datasets.TUMSequence(str(root), "desk", cam).associations == TUM_WANT
    os.remove(root / "desk" / "pose.txt")
    with pytest.raises(ValueError, match="groundtruth.txt nor pose.txt"):
        datasets.TUMSequence(str(root), "desk", cam)
    with pytest.raises(ValueError, match="zero quaternion"):
        datasets.quaternion_pose([0, 0, 0, 0, 0, 0, 0])


# ----------------------------------------------------------------------------------------------------------------------- ScanNet
@pytest.fixture()
def scannet_dir(tmp_path):
    """Four frames 0, 1, 2, 10 with 13 x 9 colour and 7 x 5 depth; the pose of frame 2 holds -inf."""
    folder = tmp_path / "scene0000_00"
    os.makedirs(folder / "pose")
    for n, k in enumerate((0, 1, 2, 10)):
        _write_color(str(folder / "color" / f"{k}.jpg"), 10 + n, size=(13, 9))
        _write_depth(str(folder / "depth" / f"{k}.png"), 100 + n)
        m = np.eye(4)
        m[1, 3] = n
        if k == 2:
            m[:] = -np.inf
        np.savetxt(folder / "pose" / f"{k}.txt", m)
    return tmp_path


def test_scannet_reader_keeps_two_sizes_and_drops_bad_poses(scannet_dir):
    cam = {**CAMERA, "image_width": 13, "image_height": 9}
    seq = datasets.ScanNetSequence(str(scannet_dir), "scene0000_00", cam)
    assert seq.size == (13, 9) and seq.depth_size == (7, 5) and len(seq) == 4
    frames = list(seq)
    assert [tuple(c.shape) for c, _, _ in frames] == [(9, 13, 3)] * 4 and [tuple(d.shape) for _, d, _ in frames] == [(5, 7)] * 4
    assert [int(c[0, 0, 0]) - 10 for c, _, _ in frames] == [0, 1, 2, 3] == [int(d[0, 0]) - 100 for _, d, _ in frames]  # 10 last
    assert [bool(torch.isfinite(p).all()) for _, _, p in frames] == [True, True, False, True]
    good = datasets.ScanNetSequence(str(scannet_dir), "scene0000_00", cam, ignore_bad=True)
    assert len(good) == 3 and good.retained == [0, 1, 3] and [float(p[1, 3]) for _, _, p in good] == [0.0, 1.0, 3.0]
    assert [int(d[0, 0]) - 100 for _, d, _ in good] == [0, 1, 3]
    assert datasets.ScanNetSequence(str(scannet_dir), "scene0000_00", cam, start=2, ignore_bad=True).retained == [3]
    with pytest.raises(ValueError, match="finite pose"):
        datasets.ScanNetSequence(str(scannet_dir), "scene0000_00", cam, start=2, end=3, ignore_bad=True)


# ------------------------------------------------------------------------------------------------------- open_sequence, runner
def _config_file(tmp_path, **data):
    section = dict(basedir=GOLDEN, gradslam_data_cfg=os.path.join(GOLDEN, "kitchen", "camera.yaml"), sequence="somewhere/else/kitchen",
                   desired_image_height=320, desired_image_width=180, start=0, end=-1, stride=1, **data)
    path = tmp_path / "config.py"
    path.write_text("from pathlib import Path\nscene = 'kitchen'\nconfig = dict(seed=3, workdir='w', run_name=scene, "
                    f"data=dict({', '.join(f'{k}={v!r}' for k, v in section.items())}), frontend=dict(max_frames=5))\n")
    return str(path)


def test_open_sequence_reads_a_data_section(tmp_path, scannet_dir):
    config = run.load_config(_config_file(tmp_path, dataset_name="Replica"))
    assert config["seed"] == 3 and config["frontend"] == dict(max_frames=5)
    seq = datasets.open_sequence(config["data"])
    assert isinstance(seq, datasets.ReplicaSequence) and len(seq) == 11 and seq.size == (360, 640)  # the last path component names it
    assert datasets.working_size(config["data"]) == (180, 320) and datasets.working_size(dict(basedir="x")) is None
    assert len(datasets.open_sequence({**config["data"], "start": 2, "end": 9, "stride": 3})) == 3
    seq, prepared = run.prepare(config, frames=4)
    assert len(seq) == 4 and prepared["cameras"] == dict(width=180, height=320) and prepared["data"]["end"] == 4
    assert "cameras" not in config and config["data"]["end"] == -1  # the loaded configuration is left as it was
    assert len(run.prepare({**config, "data": {**config["data"], "start": 1, "stride": 2}}, frames=3)[0].retained) == 3
    assert len(run.prepare({**config, "data": {**config["data"], "end": 2}}, frames=5)[0]) == 2
    # without a camera file the section names the dataset and carries the camera itself
    section = dict(dataset_name="ScanNet", basedir=str(scannet_dir), sequence="scene0000_00", ignore_bad=True,
                   camera_params={**CAMERA, "image_width": 13, "image_height": 9})
    seq = datasets.open_sequence(section)
    assert isinstance(seq, datasets.ScanNetSequence) and len(seq) == 3 and seq.depth_size == (7, 5)
    with pytest.raises(ValueError, match=r"unknown dataset name 'azure'; known: replica, tum, scannet"):
        datasets.open_sequence({**section, "dataset_name": "Azure"})
    with pytest.raises(ValueError, match="basedir"):
        datasets.open_sequence({k: v for k, v in section.items() if k != "basedir"})
    with pytest.raises(ValueError, match="frames"):
        run.prepare(config, frames=0)
    bad = tmp_path / "empty.py"
    bad.write_text("settings = {}\n")
    with pytest.raises(ValueError, match="defines no dict"):
        run.load_config(str(bad))
    with pytest.raises(ValueError, match="data"):
        run.prepare(dict(seed=1))


def test_runner_reports_a_refused_configuration(tmp_path, capsys):
    """check_config's refusal comes before anything touches the device: exit status 2 and the key's name on stderr."""
    from tests import front_ref as fr
    cfg = fr.slam_config(180, 320)
    cfg["render"]["enable_exposure"] = True
    data = run.load_config(_config_file(tmp_path))["data"]
    path = tmp_path / "refused.py"
    path.write_text(f"config = {dict(cfg, data=data)!r}\n")
    assert run.main([str(path), "--frames", "2", "--out", str(tmp_path / "out")]) == 2
    assert "enable_exposure" in capsys.readouterr().err and not os.path.exists(tmp_path / "out")


# ----------------------------------------------------------------------------------------------------------------------- writers
def test_writers_round_trip(tmp_path):
    from tests import front_ref as fr
    rng = np.random.default_rng(5)
    w2c = torch.from_numpy(fr.random_poses(rng, 6))
    path = str(tmp_path / "traj_est.txt")
    slam.write_trajectory(path, w2c)
    rows = np.loadtxt(path)
    assert rows.shape == (6, 16) and len(open(path).read().splitlines()) == 6  # the layout of traj.txt
    back = rows.reshape(6, 4, 4)
    assert np.abs(back - fr.rigid_inverse(w2c.numpy())).max() < 1e-15 and np.array_equal(back[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (6, 1)))
    assert np.abs(back @ w2c.double().numpy() - np.eye(4)).max() < 1e-5
    params = {n: torch.from_numpy(rng.normal(size=(50, k)).astype(np.float32)) for n, k in
              (("means3D", 3), ("opacities", 1), ("scales", 2), ("rotations", 4), ("colors", 3))}
    slam.write_map(str(tmp_path / "map.ply"), params)
    got = ply.load_ply(str(tmp_path / "map.ply"))
    for name, key in (("means3D", "xyz"), ("opacities", "opacity"), ("scales", "scaling"), ("rotations", "rotation"), ("colors", "rgb")):
        assert np.array_equal(got[key], params[name].numpy()), name
    evaluation = dict(psnr=np.array([30.5, 31.25]), mean_psnr=30.875, ate_rmse=0.0125, per_frame=np.zeros((2, 3)), t=torch.tensor([1.5]))
    slam.write_results(str(tmp_path / "results.json"), evaluation, dict(front="gs2d-front-hip src 0123"), dict(basedir="b", start=0), 7)
    res = json.load(open(tmp_path / "results.json"))
    assert res["evaluation"] == dict(psnr=[30.5, 31.25], mean_psnr=30.875, ate_rmse=0.0125, per_frame=[[0.0] * 3] * 2, t=[1.5])
    assert res["build"] == dict(front="gs2d-front-hip src 0123") and res["data"] == dict(basedir="b", start=0) and res["seed"] == 7
