"""CPU tests of datasets.ScanNetPPSequence on a layout the test writes itself: 5 train and 3 test images of 12x8, the train list
NOT in natural order, one train and one test image marked is_bad.  No dataset is needed and nothing is launched."""
import json
import os

import numpy as np
import pytest
import torch

from gaus_slam_amd import datasets

W, H = 12, 8
TRAIN = ["DSC00010.JPG", "DSC00002.JPG", "DSC00007.JPG", "DSC00001.JPG", "DSC00004.JPG"]  # the order of use, not the natural one
TEST = ["DSC00009.JPG", "DSC00003.JPG", "DSC00005.JPG"]
BAD = {"DSC00007.JPG", "DSC00003.JPG"}
CAMERA = dict(w=W, h=H, fl_x=10.5, fl_y=10.25, cx=5.75, cy=3.5)
P = np.diag([1.0, -1.0, -1.0, 1.0])


def c2w_of(name):
    """A rigid pose that depends on the image's number, with entries that are not float32 numbers."""
    k = int(name[3:8])
    a = 0.1 * k + 1.0 / 3.0
    m = np.eye(4)
    m[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    m[:3, 3] = [k / 7.0, -k / 3.0, 0.1 * k]
    return m


def write_tree(root, sequence="seq0", train=TRAIN, test=TEST, size=(W, H), camera=CAMERA, drop_meta=(), lists=None, meta_edit=None):
    from PIL import Image
    d = os.path.join(root, sequence, "dslr")
    for sub in ("undistorted_images", "undistorted_depths", "nerfstudio"):
        os.makedirs(os.path.join(d, sub), exist_ok=True)
    rng = np.random.default_rng(0)
    for name in train + test:
        k = int(name[3:8])
        Image.fromarray(np.full((size[1], size[0], 3), 10 * k, np.uint8)).save(os.path.join(d, "undistorted_images", name), quality=100)
        depth = (1000 + 100 * k + rng.integers(0, 50, (size[1], size[0]))).astype(np.uint16)
        Image.fromarray(depth).save(os.path.join(d, "undistorted_depths", name.replace(".JPG", ".png")))
    entry = lambda n: dict(file_path=n, transform_matrix=c2w_of(n).tolist(), is_bad=n in BAD)
    # the metadata lists the images in natural order: the lists decide the order of use
    meta = dict(camera, frames=[entry(n) for n in sorted(train) if n not in drop_meta], test_frames=[entry(n) for n in sorted(test) if n not in drop_meta])
    if meta_edit is not None:
        meta_edit(meta)
    with open(os.path.join(d, "train_test_lists.json"), "w") as fh:
        json.dump(dict(train=train, test=test) if lists is None else lists, fh)
    with open(os.path.join(d, "nerfstudio", "transforms_undistorted.json"), "w") as fh:
        json.dump(meta, fh)
    return d


def expected_pose(name):
    return (P @ c2w_of(name) @ P.T).astype(np.float32)


def names_of(seq):
    return [os.path.basename(p) for p in seq.color_paths]


def test_train_split_order_paths_poses_camera(tmp_path):
    d = write_tree(str(tmp_path))
    seq = datasets.ScanNetPPSequence(str(tmp_path), "seq0")
    assert len(seq) == 5 and names_of(seq) == TRAIN == seq.image_names
    assert seq.color_paths == [os.path.join(d, "undistorted_images", n) for n in TRAIN]
    assert seq.depth_paths == [os.path.join(d, "undistorted_depths", n.replace(".JPG", ".png")) for n in TRAIN]
    assert seq.size == (W, H) and seq.depth_size == (W, H) and seq.distortion is None
    assert seq.intrinsics == (10.5, 10.25, 5.75, 3.5) and seq.png_depth_scale == 1000.0
    frames = list(seq)
    for name, (color, depth, c2w) in zip(TRAIN, frames):
        k = int(name[3:8])
        assert color.dtype == torch.uint8 and tuple(color.shape) == (H, W, 3) and abs(int(color[0, 0, 0]) - 10 * k) <= 2
        assert depth.dtype == torch.uint16 and tuple(depth.shape) == (H, W)
        assert 1000 + 100 * k <= int(depth.view(torch.int16).min()) and int(depth.view(torch.int16).max()) < 1050 + 100 * k
        assert c2w.dtype == torch.float32 and np.array_equal(c2w.numpy(), expected_pose(name))  # narrowed once, after the product


def test_test_split_has_the_anchor_first(tmp_path):
    write_tree(str(tmp_path))
    seq = datasets.ScanNetPPSequence(str(tmp_path), "seq0", use_train_split=False)
    assert len(seq) == 1 + 3 and names_of(seq) == [TRAIN[0]] + TEST
    for name, pose in zip([TRAIN[0]] + TEST, seq.poses):
        assert np.array_equal(pose.astype(np.float32), expected_pose(name))
    # the anchor is never filtered, even when it is bad itself
    write_tree(str(tmp_path), sequence="seq1", train=["DSC00007.JPG"] + TRAIN[:2])
    seq = datasets.ScanNetPPSequence(str(tmp_path), "seq1", use_train_split=False, ignore_bad=True)
    assert names_of(seq) == ["DSC00007.JPG", "DSC00009.JPG", "DSC00005.JPG"]


def test_ignore_bad_and_slicing(tmp_path):
    write_tree(str(tmp_path))
    seq = datasets.ScanNetPPSequence(str(tmp_path), "seq0", ignore_bad=True)
    assert names_of(seq) == [n for n in TRAIN if n not in BAD] and len(seq) == 4
    seq = datasets.ScanNetPPSequence(str(tmp_path), "seq0", ignore_bad=True, use_train_split=False)
    assert names_of(seq) == [TRAIN[0], "DSC00009.JPG", "DSC00005.JPG"]
    seq = datasets.ScanNetPPSequence(str(tmp_path), "seq0", start=1, end=5, stride=2)
    assert names_of(seq) == TRAIN[1:5:2] and seq.retained == [1, 3] and seq.image_names == TRAIN[1:5:2]
    # the anchor is part of the list that is sliced, as in the reference's base class
    seq = datasets.ScanNetPPSequence(str(tmp_path), "seq0", use_train_split=False, start=0, end=-1, stride=2)
    assert names_of(seq) == [TRAIN[0], TEST[1]]
    seq = datasets.ScanNetPPSequence(str(tmp_path), "seq0", use_train_split=False, start=1)
    assert names_of(seq) == TEST
    seq = datasets.ScanNetPPSequence(str(tmp_path), "seq0", use_train_split=False, end=2)
    assert names_of(seq) == [TRAIN[0], TEST[0]]


def test_refusals(tmp_path):
    root = str(tmp_path)
    for key in ("h", "w", "fl_x", "fl_y", "cx", "cy", "frames"):
        write_tree(root, sequence="no_" + key, meta_edit=lambda m, key=key: m.pop(key))
        with pytest.raises(ValueError, match=rf"transforms_undistorted\.json lacks the key '{key}'"):
            datasets.ScanNetPPSequence(root, "no_" + key)
    write_tree(root, sequence="no_test_frames", meta_edit=lambda m: m.pop("test_frames"))
    datasets.ScanNetPPSequence(root, "no_test_frames")  # the train split does not read them
    with pytest.raises(ValueError, match=r"transforms_undistorted\.json lacks the key 'test_frames'"):
        datasets.ScanNetPPSequence(root, "no_test_frames", use_train_split=False)
    for key in ("train", "test"):
        write_tree(root, sequence="lists_" + key, lists={k: v for k, v in dict(train=TRAIN, test=TEST).items() if k != key})
        with pytest.raises(ValueError, match=rf"train_test_lists\.json lacks the key '{key}'"):
            datasets.ScanNetPPSequence(root, "lists_" + key)
    for key in ("transform_matrix", "is_bad", "file_path"):
        write_tree(root, sequence="entry_" + key, meta_edit=lambda m, key=key: m["frames"][1].pop(key))
        with pytest.raises(ValueError, match=rf"lacks the key '{key}'"):
            datasets.ScanNetPPSequence(root, "entry_" + key, ignore_bad=True)
    write_tree(root, sequence="absent", drop_meta=("DSC00007.JPG",))
    with pytest.raises(ValueError, match=r"'frames' has no entry for the image 'DSC00007\.JPG'"):
        datasets.ScanNetPPSequence(root, "absent")
    write_tree(root, sequence="absent_test", drop_meta=("DSC00003.JPG",))
    with pytest.raises(ValueError, match=r"'test_frames' has no entry for the image 'DSC00003\.JPG'"):
        datasets.ScanNetPPSequence(root, "absent_test", use_train_split=False)
    write_tree(root, sequence="all_bad", train=["DSC00007.JPG"], test=["DSC00003.JPG"])
    with pytest.raises(ValueError, match="holds no frame"):
        datasets.ScanNetPPSequence(root, "all_bad", ignore_bad=True)
    write_tree(root, sequence="no_train", train=[], test=TEST)
    with pytest.raises(ValueError, match="holds no frame"):
        datasets.ScanNetPPSequence(root, "no_train")
    with pytest.raises(ValueError, match="no anchor"):
        datasets.ScanNetPPSequence(root, "no_train", use_train_split=False)
    write_tree(root)
    with pytest.raises(ValueError, match="holds no frame"):
        datasets.ScanNetPPSequence(root, "seq0", start=7)
    with pytest.raises(ValueError, match="start must not be negative"):
        datasets.ScanNetPPSequence(root, "seq0", start=-1)
    write_tree(root, sequence="other_size", camera=dict(CAMERA, w=W + 2))
    with pytest.raises(ValueError, match="the camera says"):
        datasets.ScanNetPPSequence(root, "other_size").frame(0)


def test_open_sequence_needs_no_camera_file(tmp_path):
    write_tree(str(tmp_path))
    data = dict(dataset_name="scannetpp", basedir=str(tmp_path), sequence="somewhere/seq0", start=0, end=-1, stride=1, ignore_bad=True,
                desired_image_width=6, desired_image_height=4)
    seq = datasets.open_sequence(data)
    assert isinstance(seq, datasets.ScanNetPPSequence) and names_of(seq) == [n for n in TRAIN if n not in BAD]
    seq = datasets.open_sequence({**data, "use_train_split": False, "ignore_bad": False})
    assert names_of(seq) == [TRAIN[0]] + TEST
    assert datasets.working_size(data) == (6, 4)
    assert datasets.READERS["scannetpp"] is datasets.ScanNetPPSequence and datasets.KNOWN == ("replica", "tum", "scannet", "scannetpp")
    with pytest.raises(ValueError, match="known: replica, tum, scannet, scannetpp"):
        datasets.open_sequence({**data, "dataset_name": "kitti"})
    # the runner's preparation takes it as it takes the others
    from gaus_slam_amd import run
    seq, config = run.prepare({"data": data}, frames=2)
    assert len(seq) == 2 and config["cameras"] == {"width": 6, "height": 4}
