"""A finished run as the reference saves it (scene/__init__.py `save_scence` / `load_scence`): four files in one directory,
under the reference's names,

    config.json       the configuration, json.dump
    gaussians.ply     the map's raw parameters (ply.save_ply: the layout of map.ply)
    w2cs.npz.npy      the estimated world-to-camera poses, float32 [N,4,4] -- the name np.save("w2cs.npz", ...) produces
    gt_w2cs.npz.npy   the ground-truth ones

so that a run can be evaluated later (python -m gaus_slam_amd.nvs).  A scene saved by the reference itself has the same four
names and the same PLY attribute order and should load; no such file was ever available to try it.

    save_scene(path, config, raw_params, w2cs, gt_w2cs)
    config, raw_params, w2cs, gt_w2cs = load_scene(path)        # tensors on `device`
    params = activate(raw_params)                               # what render.render takes (gs2d_map_activate)"""
import json
import os
from collections import OrderedDict

import numpy as np
import torch

FILES = ("config.json", "gaussians.ply", "w2cs.npz.npy", "gt_w2cs.npz.npy")
PARAMS = OrderedDict((("means3D", "xyz"), ("opacities", "opacity"), ("scales", "scaling"), ("rotations", "rotation"), ("colors", "rgb")))


def _check_json(value, where):
    """Raises ValueError naming the key of the first value json cannot hold."""
    if isinstance(value, dict):
        for k, v in value.items():
            if not isinstance(k, (str, int, float, bool, type(None))):
                raise ValueError(f"config{where}: the key {k!r} is no json key")
            _check_json(v, f"{where}[{k!r}]")
    elif isinstance(value, (list, tuple)):
        for i, v in enumerate(value):
            _check_json(v, f"{where}[{i}]")
    elif not isinstance(value, (str, int, float, bool, type(None))):
        raise ValueError(f"config{where} holds a {type(value).__name__}, which json cannot hold")


def _poses(w2cs, name):
    if isinstance(w2cs, torch.Tensor):
        a = w2cs.detach().cpu().numpy()
    elif len(w2cs) and isinstance(w2cs[0], torch.Tensor):
        a = torch.stack([m.detach() for m in w2cs]).cpu().numpy()
    else:
        a = np.asarray(w2cs)
    if a.ndim != 3 or a.shape[1:] != (4, 4):
        raise ValueError(f"{name} must be [N,4,4], got {a.shape}")
    return np.ascontiguousarray(a, dtype=np.float32)


def save_scene(path, config, raw_params, w2cs, gt_w2cs):
    """Writes FILES into `path`.  raw_params: means3D, opacities, scales, rotations, colors as [P,k] tensors or arrays of RAW
    values (opacity logits, log scales, unnormalised quaternions).  w2cs, gt_w2cs: [N,4,4] tensors, arrays or lists of [4,4]."""
    from . import ply
    _check_json(config, "")
    missing = [n for n in PARAMS if n not in raw_params]
    if missing:
        raise ValueError(f"raw_params lacks {missing}")
    est, gt = _poses(w2cs, "w2cs"), _poses(gt_w2cs, "gt_w2cs")
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, FILES[0]), "w") as fh:
        json.dump(config, fh)
    host = {n: (raw_params[n].detach().cpu().numpy() if isinstance(raw_params[n], torch.Tensor) else np.asarray(raw_params[n]))
            for n in PARAMS}
    ply.save_ply(os.path.join(path, FILES[1]), host["means3D"], host["opacities"], host["scales"], host["rotations"], rgb=host["colors"])
    with open(os.path.join(path, FILES[2]), "wb") as fh:  # a file object: np.save appends no suffix of its own
        np.save(fh, est)
    with open(os.path.join(path, FILES[3]), "wb") as fh:
        np.save(fh, gt)


def load_scene(path, device="cuda"):
    """(config, raw_params, w2cs, gt_w2cs) of a directory save_scene wrote: raw_params an OrderedDict of float32 [P,k] tensors,
    the poses float32 [N,4,4], all on `device`.  Raises FileNotFoundError naming the first of the four files that is missing."""
    from . import ply
    for f in FILES:
        if not os.path.isfile(os.path.join(path, f)):
            raise FileNotFoundError(f"the scene {path} is broken: it lacks {f}")
    with open(os.path.join(path, FILES[0])) as fh:
        config = json.load(fh)
    table = ply.load_ply(os.path.join(path, FILES[1]))
    if "rgb" not in table:
        raise ValueError(f"{os.path.join(path, FILES[1])} holds SH colours, which are not supported")
    raw = OrderedDict((n, torch.from_numpy(np.ascontiguousarray(table[k], dtype=np.float32)).to(device)) for n, k in PARAMS.items())
    poses = [torch.from_numpy(np.load(os.path.join(path, f)).astype(np.float32, copy=False)).to(device) for f in FILES[2:]]
    for f, p in zip(FILES[2:], poses):
        if p.dim() != 3 or tuple(p.shape[1:]) != (4, 4):
            raise ValueError(f"{os.path.join(path, f)} holds no [N,4,4] array")
    return config, raw, poses[0], poses[1]


def activate(raw_params):
    """The activated parameters render.render and evaluate.evaluate_map take, from raw ones on the device: one launch of
    gs2d_map_activate (sigmoid, exp, normalise); means3D and colors are passed through."""
    from . import _map_lib
    from ._check import check_device, check_tensor
    P = int(raw_params["means3D"].shape[0])
    for n, k in (("means3D", 3), ("opacities", 1), ("scales", 2), ("rotations", 4), ("colors", 3)):
        check_tensor(raw_params[n], n, shape=(P, k))
    dev = raw_params["means3D"].device
    check_device(dev, *((raw_params[n], n) for n in PARAMS))
    act = {n: torch.empty_like(raw_params[n]) for n in ("opacities", "scales", "rotations")}
    _map_lib.call("gs2d_map_activate", dev, P, raw_params["opacities"].data_ptr(), raw_params["scales"].data_ptr(),
                  raw_params["rotations"].data_ptr(), act["opacities"].data_ptr(), act["scales"].data_ptr(), act["rotations"].data_ptr())
    return OrderedDict((n, act.get(n, raw_params[n])) for n in PARAMS)
