"""Readers of recorded RGB-D sequences, as sequences for slam.run_slam: plain Python on the CPU, written from the on-disk layouts
of the reference's datasets (datasets/gradslam_datasets/{replica,tum,scannet,scannetpp}.py), not from its loaders.

    seq = ReplicaSequence(basedir, "kitchen", camera)        # camera: the camera_params mapping of a camera.yaml
    seq = open_sequence(config["data"])                      # from a reference config's `data` section
    for color_u8, depth, gt_c2w in seq: ...                  # uint8 [Hc,Wc,3], uint16 [Hd,Wd], float32 [4,4] camera-to-world
    seq.intrinsics, seq.png_depth_scale, seq.size            # (fx, fy, cx, cy) at the colour size, units per metre, (Wc, Hc)
    seq.depth_size, seq.distortion                           # (Wd, Hd); None or (k1, k2, p1, p2, k3)

Nothing is resized, undistorted or scaled here: that is one launch per frame on the device (frontend_ops.ingest / ingest_ex),
which run_slam chooses by depth_size and distortion.  Images are decoded with Pillow and camera files with PyYAML, both imported
where they are first needed; a missing one raises an error that names it.  File names are ordered naturally (frame_2 before
frame_10).  start / end / stride select frames[start:end:stride] as the reference does, end == -1 meaning all, with its refusals:
ValueError for start < 0, for an end that is neither -1 nor above start, and for colour and depth lists of different lengths.
`crop_edge` of a camera file is read and ignored: the reference never applies it.

Departures: the TUM pose list is read without its comment lines and nothing else is skipped (the reference also drops the first
line, which is a comment in every published sequence); ScanNetSequence(ignore_bad=True) drops the frames of the selected range
whose pose is not finite (the reference accepts the flag and leaves such frames in)."""
import glob
import json
import math
import os
import re

import numpy as np
import torch

KNOWN = ("replica", "tum", "scannet", "scannetpp")
MAX_DT = 0.08  # seconds between a colour stamp and the depth / pose stamp associated with it (TUM)
FRAME_RATE = 32  # successive TUM frames are more than 1 / FRAME_RATE seconds apart


def _need(module, package):
    try:
        return __import__(module, fromlist=["_"])
    except ImportError as e:
        raise RuntimeError(f"gaus_slam_amd.datasets needs the {package} package, which is not installed ({e})") from e


def natural_key(path):
    """Sort key of a file name: digit runs compare as numbers."""
    return [int(t) if t.isdigit() else t for t in re.split(r"(\d+)", os.path.basename(path))]


def natural_glob(pattern):
    return sorted(glob.glob(pattern), key=natural_key)


def quaternion_pose(vec):
    """tx ty tz qx qy qz qw -> float64 [4,4] camera-to-world; the quaternion is normalised first."""
    tx, ty, tz, x, y, z, w = (float(v) for v in vec)
    n = math.sqrt(x * x + y * y + z * z + w * w)
    if not n > 0:
        raise ValueError(f"a pose has the zero quaternion: {list(vec)}")
    x, y, z, w = x / n, y / n, z / n, w / n
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), tx],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w), ty],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y), tz],
                     [0.0, 0.0, 0.0, 1.0]], np.float64)


def load_camera(path):
    """The mapping of a camera.yaml / configs/data/*.yaml: {'dataset_name': ..., 'camera_params': {...}}."""
    yaml = _need("yaml", "PyYAML")
    with open(path) as fh:
        cfg = yaml.safe_load(fh)
    if not isinstance(cfg, dict) or "camera_params" not in cfg:
        raise ValueError(f"{path} holds no camera_params")
    if cfg.get("inherit_from") is not None:
        raise ValueError(f"{path}: inherit_from is not supported; write the camera parameters into one file")
    return cfg


def associate(t_color, t_depth, t_pose, max_dt=MAX_DT, frame_rate=FRAME_RATE):
    """[(i, j, k)]: for every colour stamp the nearest depth and the nearest pose, each less than max_dt away, then thinned so
    that the colour stamps of successive entries are more than 1 / frame_rate apart."""
    t_color, t_depth, t_pose = (np.asarray(t, np.float64) for t in (t_color, t_depth, t_pose))
    pairs = []
    for i, t in enumerate(t_color):
        j, k = int(np.argmin(np.abs(t_depth - t))), int(np.argmin(np.abs(t_pose - t)))
        if abs(t_depth[j] - t) < max_dt and abs(t_pose[k] - t) < max_dt:
            pairs.append((i, j, k))
    kept = pairs[:1]
    for p in pairs[1:]:
        if t_color[p[0]] - t_color[kept[-1][0]] > 1.0 / frame_rate:
            kept.append(p)
    return kept


def _rows(path):
    """The whitespace-separated fields of every line that is neither empty nor a comment."""
    with open(path) as fh:
        return [ln.split() for ln in fh if ln.strip() and not ln.lstrip().startswith("#")]


class RecordedSequence:
    """What the readers share: the camera, the frame selection and the decoding of one frame."""

    def __init__(self, camera, color_paths, depth_paths, poses, start=0, end=-1, stride=1):
        camera = camera.get("camera_params", camera)
        for key in ("image_height", "image_width", "fx", "fy", "cx", "cy", "png_depth_scale"):
            if key not in camera:
                raise ValueError(f"the camera parameters lack {key!r}")
        self.size = (int(camera["image_width"]), int(camera["image_height"]))
        self.intrinsics = tuple(float(camera[k]) for k in ("fx", "fy", "cx", "cy"))
        self.png_depth_scale = float(camera["png_depth_scale"])
        self.crop_edge = camera.get("crop_edge")  # read, never applied
        self.distortion = None
        if camera.get("distortion") is not None:
            d = [float(v) for v in camera["distortion"]]
            if len(d) not in (4, 5):
                raise ValueError(f"distortion must hold k1 k2 p1 p2 [k3], got {len(d)} values")
            self.distortion = tuple(d + [0.0] * (5 - len(d)))
        start, end, stride = int(start), int(end), 1 if stride is None else int(stride)
        if start < 0:
            raise ValueError(f"start must not be negative, got {start}")
        if not (end == -1 or end > start):
            raise ValueError(f"end ({end}) must be -1 (all frames) or greater than start ({start})")
        if stride < 1:
            raise ValueError(f"stride must be >= 1, got {stride}")
        if len(color_paths) != len(depth_paths):
            raise ValueError(f"the numbers of colour ({len(color_paths)}) and depth ({len(depth_paths)}) images must be the same")
        if len(poses) < len(color_paths):
            raise ValueError(f"{len(color_paths)} frames but only {len(poses)} poses")
        pick = slice(start, len(color_paths) if end == -1 else end, stride)
        self.color_paths, self.depth_paths = list(color_paths)[pick], list(depth_paths)[pick]
        self.poses = [np.asarray(p, np.float64).reshape(4, 4) for p in list(poses)[:len(color_paths)][pick]]
        self.retained = list(range(len(color_paths)))[pick]  # the indices of the kept frames in the unselected lists
        if not self.color_paths:
            raise ValueError("the selection holds no frame")
        self._depth_size = None

    def __len__(self):
        return len(self.color_paths)

    @property
    def depth_size(self):
        """(Wd, Hd) of the first depth image (its header only is read)."""
        if self._depth_size is None:
            Image = _need("PIL.Image", "Pillow")
            with Image.open(self.depth_paths[0]) as im:
                self._depth_size = (int(im.size[0]), int(im.size[1]))
        return self._depth_size

    def frame(self, k):
        """(color_u8 [Hc,Wc,3] uint8, depth [Hd,Wd] uint16, gt_c2w float32 [4,4]) of frame k, as stored."""
        Image = _need("PIL.Image", "Pillow")
        with Image.open(self.color_paths[k]) as im:
            color = np.array(im.convert("RGB"), np.uint8)  # a copy: torch wants writable memory
        if (color.shape[1], color.shape[0]) != self.size:
            raise ValueError(f"{self.color_paths[k]} is {color.shape[1]} x {color.shape[0]}, the camera says {self.size[0]} x {self.size[1]}")
        with Image.open(self.depth_paths[k]) as im:
            depth = np.asarray(im)
        if depth.ndim != 2 or depth.dtype.kind not in "ui" or int(depth.min()) < 0 or int(depth.max()) > 65535:
            raise ValueError(f"{self.depth_paths[k]} is not a single-channel 16-bit depth image")
        if (depth.shape[1], depth.shape[0]) != self.depth_size:
            raise ValueError(f"{self.depth_paths[k]} is {depth.shape[1]} x {depth.shape[0]}, the first depth image {self.depth_size}")
        return (torch.from_numpy(np.ascontiguousarray(color)), torch.from_numpy(np.ascontiguousarray(depth).astype(np.uint16)),
                torch.from_numpy(self.poses[k]).float())

    def __iter__(self):
        return (self.frame(k) for k in range(len(self)))


class ReplicaSequence(RecordedSequence):
    """<basedir>/<sequence>/results/frame*.jpg and depth*.png in natural order; traj.txt: one row-major 4x4 camera-to-world pose
    per line, line i for frame i."""

    def __init__(self, basedir, sequence, camera, start=0, end=-1, stride=1):
        folder = os.path.join(basedir, sequence)
        colors = natural_glob(os.path.join(folder, "results", "frame*.jpg"))
        depths = natural_glob(os.path.join(folder, "results", "depth*.png"))
        poses = [np.array([float(v) for v in row], np.float64) for row in _rows(os.path.join(folder, "traj.txt"))]
        if any(p.size != 16 for p in poses):
            raise ValueError(f"{folder}/traj.txt: every line must hold 16 numbers")
        super().__init__(camera, colors, depths, poses, start, end, stride)


class TUMSequence(RecordedSequence):
    """<basedir>/<sequence>/rgb.txt and depth.txt (stamp, file), groundtruth.txt or pose.txt (stamp tx ty tz qx qy qz qw, camera to
    world), associated and thinned by associate()."""

    def __init__(self, basedir, sequence, camera, start=0, end=-1, stride=1):
        folder = os.path.join(basedir, sequence)
        pose_list = next((p for p in (os.path.join(folder, n) for n in ("groundtruth.txt", "pose.txt")) if os.path.isfile(p)), None)
        if pose_list is None:
            raise ValueError(f"{folder} holds neither groundtruth.txt nor pose.txt")
        rgb, dep, pos = _rows(os.path.join(folder, "rgb.txt")), _rows(os.path.join(folder, "depth.txt")), _rows(pose_list)
        stamps = lambda rows: [float(r[0]) for r in rows]
        self.associations = associate(stamps(rgb), stamps(dep), stamps(pos))
        colors = [os.path.join(folder, rgb[i][1]) for i, _, _ in self.associations]
        depths = [os.path.join(folder, dep[j][1]) for _, j, _ in self.associations]
        poses = [quaternion_pose(pos[k][1:8]) for _, _, k in self.associations]
        super().__init__(camera, colors, depths, poses, start, end, stride)


class ScanNetSequence(RecordedSequence):
    """<basedir>/<sequence>/color/*.jpg, depth/*.png and pose/*.txt (one 4x4 camera-to-world per file), each in natural order.
    The colour and depth sizes differ (1296 x 968 against 640 x 480).  ignore_bad: drop the selected frames whose pose is not
    finite."""

    def __init__(self, basedir, sequence, camera, start=0, end=-1, stride=1, ignore_bad=False):
        folder = os.path.join(basedir, sequence)
        colors = natural_glob(os.path.join(folder, "color", "*.jpg"))
        depths = natural_glob(os.path.join(folder, "depth", "*.png"))
        poses = [np.loadtxt(p, dtype=np.float64) for p in natural_glob(os.path.join(folder, "pose", "*.txt"))]
        if any(p.size != 16 for p in poses):
            raise ValueError(f"{folder}/pose: every file must hold a 4x4 matrix")
        super().__init__(camera, colors, depths, poses, start, end, stride)
        if ignore_bad:
            good = [k for k, p in enumerate(self.poses) if np.isfinite(p).all()]
            if not good:
                raise ValueError("no selected frame has a finite pose")
            for name in ("color_paths", "depth_paths", "poses", "retained"):
                setattr(self, name, [getattr(self, name)[k] for k in good])


class ScanNetPPSequence(RecordedSequence):
    """<basedir>/<sequence>/dslr: train_test_lists.json names the `train` and `test` images, in the order they are used (not the
    natural one); nerfstudio/transforms_undistorted.json holds the camera (h, w, fl_x, fl_y, cx, cy) and, under `frames` for the
    train and `test_frames` for the test images, one entry per image with file_path, transform_matrix (4x4) and is_bad.  Colour is
    undistorted_images/<name>, depth undistorted_depths/<name with .JPG replaced by .png>, in millimetres (png_depth_scale 1000);
    no camera file is needed.  The pose is P @ transform_matrix @ P.T with P = diag(1, -1, -1, 1), in float64.
    use_train_split=False yields the FIRST TRAIN IMAGE first, never filtered by is_bad, then the test list: relative to that
    anchor the held-out poses land in the frame of a map built from the train split.  ignore_bad drops the listed images whose
    entry has is_bad true.  start / end / stride slice the resulting list, anchor included."""

    def __init__(self, basedir, sequence, camera=None, start=0, end=-1, stride=1, ignore_bad=False, use_train_split=True):
        folder = os.path.join(basedir, sequence, "dslr")
        lists_path = os.path.join(folder, "train_test_lists.json")
        meta_path = os.path.join(folder, "nerfstudio", "transforms_undistorted.json")
        with open(lists_path) as fh:
            lists = json.load(fh)
        with open(meta_path) as fh:
            meta = json.load(fh)

        def key(mapping, name, path):
            if not isinstance(mapping, dict) or name not in mapping:
                raise ValueError(f"{path} lacks the key {name!r}")
            return mapping[name]

        train, test = list(key(lists, "train", lists_path)), list(key(lists, "test", lists_path))
        cam = {"png_depth_scale": 1000.0}  # millimetres
        for ours, theirs in (("image_height", "h"), ("image_width", "w"), ("fx", "fl_x"), ("fy", "fl_y"), ("cx", "cx"), ("cy", "cy")):
            cam[ours] = key(meta, theirs, meta_path)
        P = np.diag([1.0, -1.0, -1.0, 1.0])

        def entries(group):
            return {key(e, "file_path", f"{meta_path}: an entry of {group!r}"): e for e in key(meta, group, meta_path)}

        def entry(table, group, name):
            if name not in table:
                raise ValueError(f"{meta_path}: {group!r} has no entry for the image {name!r} that {lists_path} lists")
            return table[name]

        def pose(e, group):
            m = np.asarray(key(e, "transform_matrix", f"{meta_path}: an entry of {group!r}"), np.float64)
            if m.shape != (4, 4):
                raise ValueError(f"{meta_path}: the transform_matrix of {e.get('file_path')!r} is not 4x4")
            return P @ m @ P.T

        train_table = entries("frames")
        names, poses = [], []
        if use_train_split:
            listed, table, group = train, train_table, "frames"
        else:
            listed, table, group = test, entries("test_frames"), "test_frames"
            if not train:
                raise ValueError(f"{lists_path}: the train list is empty, so there is no anchor frame")
            names.append(train[0])
            poses.append(pose(entry(train_table, "frames", train[0]), "frames"))
        for name in listed:
            e = entry(table, group, name)
            if ignore_bad and key(e, "is_bad", f"{meta_path}: the entry of {name!r}"):
                continue
            names.append(name)
            poses.append(pose(e, group))
        if not names:
            raise ValueError(f"{lists_path}: the selection holds no frame")
        self.image_names = names
        colors = [os.path.join(folder, "undistorted_images", n) for n in names]
        depths = [os.path.join(folder, "undistorted_depths", n.replace(".JPG", ".png")) for n in names]
        super().__init__(cam, colors, depths, poses, start, end, stride)
        self.image_names = [names[k] for k in self.retained]


PREFETCH_THREAD = "gaus_slam_amd.datasets.prefetch"  # the name of every reader thread prefetch() starts


def prefetch(sequence, depth=2):
    """A generator over the frames of `sequence`, in order -- sequence.frame(k) for k < len(sequence) where the reader has that
    method, else its items as iteration gives them -- read ahead by ONE daemon thread through a queue of `depth` entries, so
    that decoding frame k + 1 (Pillow releases the interpreter lock inside its decoders) overlaps what the consumer does with
    frame k.  The thread only reads: it touches no GPU and calls nothing of torch's device API.  An exception in the reader
    travels through the queue and is raised in the consumer at the position of the frame that caused it, after every frame
    before it.  Closing the generator, or dropping it, tells the thread to stop and empties the queue, so a reader blocked on a
    full queue wakes, sees the flag and ends after at most the frame it is decoding; the generator waits for that.  depth=0 is
    plain iteration, without a thread."""
    import queue
    import threading
    depth = int(depth)
    if depth < 0:
        raise ValueError(f"depth must be >= 0, got {depth}")

    def items():
        if hasattr(sequence, "frame") and hasattr(sequence, "__len__"):
            return (sequence.frame(k) for k in range(len(sequence)))
        return iter(sequence)

    if depth == 0:
        yield from items()
        return
    q, stop = queue.Queue(maxsize=depth), threading.Event()
    ITEM, END, ERROR = 0, 1, 2

    def reader():
        try:
            for item in items():
                q.put((ITEM, item))
                if stop.is_set():
                    return
            q.put((END, None))
        except BaseException as e:  # handed to the consumer, whatever it is
            q.put((ERROR, e))

    thread = threading.Thread(target=reader, name=PREFETCH_THREAD, daemon=True)
    thread.start()
    try:
        while True:
            kind, value = q.get()
            if kind == END:
                return
            if kind == ERROR:
                raise value
            yield value
    finally:
        stop.set()
        while thread.is_alive():  # every put that was waiting for room gets it; the reader then sees the flag
            try:
                q.get_nowait()
            except queue.Empty:
                thread.join(0.001)


READERS = {"replica": ReplicaSequence, "tum": TUMSequence, "scannet": ScanNetSequence, "scannetpp": ScanNetPPSequence}


def working_size(data_cfg):
    """(W, H) from desired_image_width / desired_image_height of a `data` section, or None when it names neither."""
    if "desired_image_width" not in data_cfg and "desired_image_height" not in data_cfg:
        return None
    return int(data_cfg["desired_image_width"]), int(data_cfg["desired_image_height"])


def open_sequence(data_cfg):
    """A reader from the `data` section of a reference configuration: gradslam_data_cfg (the camera file, which also names the
    dataset; without it dataset_name of the section itself), basedir, sequence (its last path component), start, end, stride,
    ignore_bad and, for ScanNet++ (which needs no camera file), use_train_split.  desired_image_width / height do not touch the reader: working_size() hands them to config['cameras']."""
    if "gradslam_data_cfg" in data_cfg:
        cam = load_camera(data_cfg["gradslam_data_cfg"])
    else:
        cam = {"dataset_name": data_cfg.get("dataset_name"), "camera_params": data_cfg.get("camera_params", {})}
    name = str(cam.get("dataset_name", data_cfg.get("dataset_name"))).lower()
    if name not in READERS:
        raise ValueError(f"unknown dataset name {name!r}; known: {', '.join(KNOWN)}")
    for key in ("basedir", "sequence"):
        if key not in data_cfg:
            raise ValueError(f"the data section lacks {key!r}")
    kw = dict(start=data_cfg.get("start", 0), end=data_cfg.get("end", -1), stride=data_cfg.get("stride", 1))
    if name in ("scannet", "scannetpp"):
        kw["ignore_bad"] = bool(data_cfg.get("ignore_bad", False))
    if name == "scannetpp":
        kw["use_train_split"] = bool(data_cfg.get("use_train_split", True))
    return READERS[name](str(data_cfg["basedir"]), os.path.basename(str(data_cfg["sequence"])), cam["camera_params"], **kw)
