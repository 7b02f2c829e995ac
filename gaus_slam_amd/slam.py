"""The whole SLAM on the device: the reference's Frontend (slam/Frontend.py), Backend (slam/Backend.py), LocalMap / Localmaps
(scene/Frame.py) and the loop of scripts/gaus.py, in plain Python on the modules of this package.

    result = run_slam(sequence, config, seed=0)
    result.trajectory(), result.gt_trajectory()      # [N,4,4] world-to-camera, on the device
    result.evaluate()                                 # evaluate.evaluate_map over the saved frames, with the ATE
    result.save(directory, data=..., seed=0)          # results.json, traj_est.txt, traj_gt.txt, map.ply (gaus_slam_amd/run.py)

`config` is a dict with the reference's key names (configs/*/config*.py); check_config() lists what is read and refuses, by name,
what the driver does not wire.  The per-frame path reads the host where the reference's control flow needs it and nowhere else:
FrameState.decide (one 32-byte read per tracked frame: lost / keyframe / new local map), the seed and prune counts of the map
modules, and the rasterizer's own read per forward.  Poses, velocities, the local-map hand-over and every camera set-up stay on
the device (frontend_ops).

Departures from the reference: the covisible submaps come from the geometric keyframe bank (covis.py), not NetVLAD; inverses of
poses are the rigid closed form; process_final() passes the frontend's tracking flag on, which the reference drops there; the
frame that closes a tracked frame is rendered with the fused tracking render, not Renderer_view."""
import json
import os
import random
from collections import OrderedDict

import torch

from . import frontend_ops as _ops
from ._check import require
from .tsdf import _intrinsics4

REFUSED = (("render", "method", lambda v: v != "2dgs"), ("gaussians", "gaussian_distribution", lambda v: v != "anisotropic"),
           ("loss", "use_normal_loss", bool), ("render", "enable_exposure", bool), ("frontend", "additional_densify", bool),
           ("backend", "gs_densify", bool))
DEFAULTS = {("render", "method"): "2dgs", ("gaussians", "gaussian_distribution"): "anisotropic"}
READ = {
    "cameras": ("height", "width", "intrinsics", "adam_betas", "frontend_lr", "backend_lr"),
    "render": ("use_sa", "use_weight_norm", "eps", "depth_near", "depth_far"),
    "frontend": ("num_tracking_iters", "num_mapping_iters", "converged_th", "tau_k", "tau_l", "max_frames", "vel_pose_init",
                 "enable_retracking"),
    "backend": ("num_ba_iters", "num_frame_saved", "num_covis_submaps", "final_refinement"),
    "densify": ("sil_thres", "scale_max"),
    "loss": ("silmask_th", "ignore_outliners", "tracking", "mapping"),
    "gaussians": ("training_args",),
}


def check_config(config):
    """Raises RuntimeError, naming the key, for a configuration the driver does not run and for a key it reads that is missing."""
    require(isinstance(config, dict), "config must be a dict")
    for section, key, bad in REFUSED:
        value = config.get(section, {}).get(key, DEFAULTS.get((section, key), False))
        require(not bad(value), f"config[{section!r}][{key!r}] = {value!r} is not supported by the driver")
    for section, keys in READ.items():
        require(isinstance(config.get(section), dict), f"config lacks the section {section!r}")
        for key in keys:
            require(key in config[section], f"config[{section!r}] lacks {key!r}")
    for key in ("xyz_lr", "opacity_lr", "scaling_lr", "rotation_lr", "rgb_lr"):
        require(key in config["gaussians"]["training_args"], f"config['gaussians']['training_args'] lacks {key!r}")
    require(int(config["backend"]["num_frame_saved"]) >= 2, "config['backend']['num_frame_saved'] must be >= 2: the first and the "
            "second-to-last frame of a local map stand for it in the keyframe bank")


def select_saved_frames(frame_types, num_saved, rng):
    """LocalMap.__init__'s choice of the frames that keep their images (scene/Frame.py:210-218), as a pure function.
    frame_types: the type of every frame of the local map, the closing one included (0 reference keyframe, 1 keyframe, 2 other);
    the candidates are frames[:-1].  Priority: rng.randint(0, 100) per candidate, + 400 for the first and the last candidate,
    + 200 for a type < 2; sorted stably, descending; the first min(num_saved, candidates) are kept."""
    n = len(frame_types) - 1
    require(n >= 1, "a local map hands over at least two frames")
    pri = [rng.randint(0, 100) for _ in range(n)]
    pri[0] += 400
    pri[-1] += 400
    pri = [(frame_types[i] < 2) * 200 + pri[i] for i in range(n)]
    return sorted(range(n), reverse=True, key=lambda i: pri[i])[:min(int(num_saved), n)]


def _lrs(config):
    t = config["gaussians"]["training_args"]
    return {name: float(t[f"{name}_lr"]) for name in ("xyz", "opacity", "scaling", "rotation", "rgb")}


def _render_kw(config):
    r = config["render"]
    return dict(use_weight_norm=bool(r["use_weight_norm"]), eps=float(r["eps"]), depth_near=float(r["depth_near"]),
                depth_far=float(r["depth_far"]))


def _mapping_kw(config):
    d = config["densify"]
    return dict(use_edge_growth=bool(d.get("use_edge_growth", False)), edge_thres=float(d.get("edge_thres", 0.4)), **_render_kw(config))


def _tracking_kw(config):
    return dict(silmask_th=float(config["loss"]["silmask_th"]), ignore_outliers=bool(config["loss"]["ignore_outliners"]),
                **_render_kw(config))


def _cull(config, name):
    d = config["densify"]
    return d[name + "_cuil"] if name + "_cuil" in d else d[name + "_cull"]


def _detached(leaves):
    """The five operator inputs without autograd: the tracking render then takes its pose-only backward."""
    return tuple(leaves[n].detach() for n in ("means3D", "opacities", "colors", "scales", "rotations"))


class Frame:
    """One frame of a local map: its images, its ground-truth pose and its frame type (0 reference keyframe, 1 keyframe, 2 other).
    est_w2c is a float32 [4,4] device tensor in the local map's frame."""

    def __init__(self, time_idx, gt_color, gt_depth, gt_w2c, frame_type):
        self.time_idx, self.gt_color, self.gt_depth, self.gt_w2c, self.frame_type = time_idx, gt_color, gt_depth, gt_w2c, frame_type
        self.est_w2c = None


class LocalMapRecord:
    """What the frontend hands to the backend (the reference's LocalMap): frames, saved_idxs, ref2f0, est_w2c [n,4,4] =
    est_w2c[k] . inv(ref2f0), the local map's raw parameters and tracking_ok.  The backend adds opt (the submap's PoseOptimizer),
    retrack_opt and its bank slots."""

    def __init__(self, lmid, frames, saved_idxs, ref2f0, est_w2c, params, tracking_ok):
        self.lmid, self.frames, self.saved_idxs, self.ref2f0, self.est_w2c = lmid, frames, saved_idxs, ref2f0, est_w2c
        self.params, self.tracking_ok = params, tracking_ok
        self.gt_w2c = torch.stack([f.gt_w2c for f in frames])
        self.opt = self.retrack_opt = None
        self.slots = []  # (bank slot, frame index)


class _Base:
    def __init__(self, config, rng, device):
        check_config(config)
        self.config, self.rng = config, rng
        device = torch.device(device)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device.index is None else device
        cam = config["cameras"]
        self.W, self.H = int(cam["width"]), int(cam["height"])
        self.intr = _intrinsics4(cam["intrinsics"])
        fx, fy, cx, cy = self.intr
        self.K = torch.tensor([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], dtype=torch.float32)  # on the host: no read
        self.use_sa = bool(config["render"]["use_sa"])
        self.eye = torch.eye(4, dtype=torch.float32, device=self.device)
        self.track_settings = self.cameras(self.eye)[0]  # the identity view of tracking.render_tracking
        self.lrs = _lrs(config)

    def cameras(self, A, B=None, **kw):
        return _ops.cameras(self.W, self.H, self.intr, A, B, use_sa=self.use_sa, **kw)

    def _tracking_step(self, opt, leaves, frame):
        """One pose-only iteration at opt.w2c against `frame`; leaves .w2c.grad behind."""
        from . import loss as _loss, tracking
        w = self.config["loss"]["tracking"]
        opt.zero_grad()
        pkg = tracking.render_tracking(self.track_settings, opt.w2c, *leaves)
        _, g_color, g_allmap = _loss.tracking_loss_and_grads(pkg["render_color"], pkg["allmap"], frame.gt_color, frame.gt_depth,
                                                             float(w["color"]), float(w["depth"]), **_tracking_kw(self.config))
        torch.autograd.backward([pkg["render_color"], pkg["allmap"]], [g_color, g_allmap])


class Frontend(_Base):
    """Frontend of the reference: tracks every frame against the current local map, grows the map at keyframes and closes it when
    tracking is lost, the map holds more than max_frames frames or more than tau_l Gaussians."""

    def __init__(self, config, rng, device="cuda"):
        super().__init__(config, rng, device)
        self.state = _ops.FrameState(self.device)
        self.local_frames, self.map, self.cur_lmid, self.tracking_flag = [], None, 0, True
        self.decisions = []  # (time_idx, Decision) of every tracked frame

    # ------------------------------------------------------------------------------------------------------------------ pieces
    def _create_map(self):
        from . import localmap
        f = self.local_frames[0]
        self.map = localmap.create_map(f.gt_color, f.gt_depth, self.K, self.lrs)
        self._mapping()

    def _mapping(self):
        from . import mapping
        frames, n = self.local_frames, int(self.config["frontend"]["num_mapping_iters"])
        if n < 1 or self.map.soa.P == 0:
            return
        settings = self.cameras(torch.stack([f.est_w2c for f in frames]))
        order = [self.rng.randrange(len(frames)) for _ in range(n)]  # random.choice(frames), Frontend.py:121
        w = self.config["loss"]["mapping"]
        mapping.map_frames(self.map, [(s, f.gt_color, f.gt_depth) for s, f in zip(settings, frames)], n, float(w["color"]),
                           float(w["depth"]), float(w["dist"]), order=order, **_mapping_kw(self.config))

    def _close(self, tracking_ok):
        from . import localmap
        frames = self.local_frames
        saved = select_saved_frames([f.frame_type for f in frames], self.config["backend"]["num_frame_saved"], self.rng)
        est = torch.stack([f.est_w2c for f in frames])
        ref2f0 = est[0].clone()
        rel = _ops.compose(est, ref2f0, inv_b=True)  # est_w2c[k] . inv(ref2f0) for every frame: one launch
        for k, f in enumerate(frames):
            f.est_w2c = rel[k]
            if k not in saved:
                f.gt_color = f.gt_depth = None
        return LocalMapRecord(self.cur_lmid, frames, saved, ref2f0, rel, localmap.extract_params(self.map), tracking_ok)

    # ---------------------------------------------------------------------------------------------------------------- pipeline
    def _gt_w2c(self, gt_pose):
        return _ops.compose(gt_pose, inv_a=True)[0]

    def _track(self, cur, last):
        """Tracks `cur` against the local map from state.next_init, renders once at the final pose and closes the frame on the
        device; sets cur.est_w2c.  Returns (Decision, that render)."""
        from . import pose as _pose, tracking
        cfg, fe = self.config, self.config["frontend"]
        opt = _pose.PoseOptimizer(self.state.next_init, cfg["cameras"]["frontend_lr"], betas=tuple(cfg["cameras"]["adam_betas"]),
                                  converged_th=max(float(fe["converged_th"]), 0.0))
        leaves = _detached(self.map.render_leaves())
        w = cfg["loss"]["tracking"]
        _pose.track(self.track_settings, opt, *leaves, cur.gt_color, cur.gt_depth, float(w["color"]), float(w["depth"]),
                    int(fe["num_tracking_iters"]), **_tracking_kw(cfg))
        w2c = opt.w2c.detach()
        with torch.no_grad():
            pkg = tracking.render_tracking(self.track_settings, w2c, *leaves)
        stats = _pose.frame_stats(pkg["allmap"], cur.gt_depth, **_render_kw(cfg))
        d = self.state.decide(stats, w2c, numel=self.H * self.W, n_local_frames=len(self.local_frames), map_size=self.map.soa.P, cfg=fe)
        cur.est_w2c = w2c.clone() if d.ok else last.est_w2c.clone()
        return d, pkg

    def _grow(self, cur, pkg):
        """A keyframe: add_new_gaussians from the render of _track, mapping, prune (Frontend.py:191-194)."""
        from . import densify
        cfg = self.config
        densify.add_new_gaussians(self.map, pkg["allmap"], cur.gt_color, cur.gt_depth, self.K, cur.est_w2c, cfg["densify"], cfg["render"])
        self._mapping()
        densify.prune_gaussians(self.map, _cull(cfg, "opacity"), _cull(cfg, "scale"), cfg["densify"]["scale_max"])

    def process_frame(self, time_idx, gt_color, gt_depth, gt_pose):
        """Frontend.process_frame (Frontend.py:142-222).  gt_color [H,W,3], gt_depth [H,W], gt_pose: camera-to-world [4,4], all
        float32 on the device.  Returns a LocalMapRecord when this frame closed a local map, else None."""
        gt_w2c = self._gt_w2c(gt_pose)
        cur = Frame(time_idx, gt_color, gt_depth, gt_w2c, 2)
        self.local_frames.append(cur)
        if len(self.local_frames) == 1:
            cur.frame_type, cur.est_w2c = 0, self.eye.clone()
            self._create_map()
            return None
        d, pkg = self._track(cur, self.local_frames[-2])
        self.decisions.append((time_idx, d))
        if d.keyframe:
            cur.frame_type = 1
            self._grow(cur, pkg)
        if not d.refkf:
            return None
        record = self._close(self.tracking_flag)
        self.cur_lmid += 1
        first = Frame(time_idx, gt_color, gt_depth, gt_w2c, 0)  # the closing frame is frame 0 of the next map, at the identity
        first.est_w2c = self.eye.clone()
        self.local_frames = [first]
        self._create_map()
        self.tracking_flag = d.ok
        return record

    def process_final(self):
        """Hands the open local map over when it holds more than one frame (Frontend.py:224-229)."""
        if len(self.local_frames) <= 1:
            return None
        record = self._close(self.tracking_flag)
        self.cur_lmid += 1
        self.local_frames = []
        return record


class Backend(_Base):
    """Backend of the reference with multi_process=False: merges every local map into the global map and runs the task list of
    covis.backend_schedule on it."""

    def __init__(self, config, rng, device="cuda"):
        from . import covis
        from .ba_shard import BUCKET_FIELDS
        from .mapping import RawGaussianAdam
        from .optim import GaussianSoA
        super().__init__(config, rng, device)
        empty = {n: torch.empty((0, k), dtype=torch.float32, device=self.device) for n, k in BUCKET_FIELDS.items()}
        self.map = RawGaussianAdam(GaussianSoA(empty), self.lrs)
        self.bank = covis.KeyframeBank(self.W, self.H, self.intr, device=self.device)
        self.local_maps = []
        self.merge_rows, self.pruned = [], 0  # what every merge returned; rows pruned since the last merge
        self.mapping_iters = 0

    # ------------------------------------------------------------------------------------------------------------------ poses
    def _transforms(self):
        """The submaps' transforms T[lm], [n_maps,4,4] on the device."""
        return torch.stack([lm.opt.matrix() for lm in self.local_maps])

    def _update_bank(self, lms):
        for i in sorted(set(lms)):
            lm = self.local_maps[i]
            w2c = _ops.compose(lm.est_w2c, lm.opt.matrix(), ia=[f for _, f in lm.slots])
            for k, (slot, _) in enumerate(lm.slots):
                self.bank.set_w2c(slot, w2c[k])

    def _pose_steps(self, opt, lm, frame_ids):
        """Pose-only steps of `opt` (the transform of submap lm) against the saved frames frame_ids, one per step:
        w2c = est_w2c[f] . T (Backend.tracking, Backend.py:81-99)."""
        leaves = _detached(self.map.render_leaves())
        with torch.no_grad():  # the factor of the first render
            opt.w2c.copy_(_ops.compose(lm.est_w2c[frame_ids[0]], opt.matrix())[0])
        for i, f in enumerate(frame_ids):
            self._tracking_step(opt, leaves, lm.frames[f])
            nxt = frame_ids[i + 1] if i + 1 < len(frame_ids) else f
            opt.step(left=lm.est_w2c[f], next_left=lm.est_w2c[nxt])

    # ------------------------------------------------------------------------------------------------------------------ tasks
    def _run_mapping(self, lms):
        """One map_frames over the draws (submap, saved frame) of a run of "mapping" tasks (Backend.mapping, Backend.py:101-128);
        the settings of all its iterations come from one cameras launch: est_w2c[f] . T[lm]."""
        from . import mapping
        if not lms or self.map.soa.P == 0:
            return
        offsets, o = [], 0
        for lm in self.local_maps:
            offsets.append(o)
            o += len(lm.frames)
        est_all = torch.cat([lm.est_w2c for lm in self.local_maps])
        draws = [(i, self.rng.choice(self.local_maps[i].saved_idxs)) for i in lms]
        settings = self.cameras(est_all, self._transforms(), ia=[offsets[i] + f for i, f in draws], ib=[i for i, _ in draws])
        frames = [(s, self.local_maps[i].frames[f].gt_color, self.local_maps[i].frames[f].gt_depth) for s, (i, f) in zip(settings, draws)]
        w = self.config["loss"]["mapping"]
        mapping.map_frames(self.map, frames, len(frames), float(w["color"]), float(w["depth"]), float(w["dist"]),
                           order=list(range(len(frames))), **_mapping_kw(self.config))
        self.mapping_iters += len(frames)

    def _run_tracking(self, lms):
        start = 0
        while start < len(lms):  # sub-runs of one submap share its optimiser
            end = start
            while end < len(lms) and lms[end] == lms[start]:
                end += 1
            lm = self.local_maps[lms[start]]
            self._pose_steps(lm.opt, lm, [self.rng.choice(lm.saved_idxs) for _ in range(end - start)])
            start = end
        self._update_bank(lms)

    def _run(self, tasks):
        from . import densify
        i = 0
        while i < len(tasks):
            kind = tasks[i][0]
            j = i
            while j < len(tasks) and tasks[j][0] == kind:
                j += 1
            lms = [lm for _, lm in tasks[i:j]]
            if kind == "mapping":
                self._run_mapping(lms)
            elif kind == "tracking":
                self._run_tracking(lms)
            else:
                require(kind == "prune", f"unknown task {kind!r}")
                cfg = self.config
                self.pruned += densify.prune_gaussians(self.map, _cull(cfg, "opacity"), _cull(cfg, "scale"), cfg["densify"]["scale_max"])
            i = j

    # --------------------------------------------------------------------------------------------------------------- pipeline
    def process_localmap(self, lm):
        """Backend.process_localmap (Backend.py:196-246) with multi_process=False."""
        from . import covis, localmap, pose as _pose
        cfg, be = self.config, self.config["backend"]
        lmid = len(self.local_maps)
        self.local_maps.append(lm)
        if lmid == 0:
            w2kf = self.eye.clone()
        else:
            last = self.local_maps[lmid - 1]
            w2kf = _ops.compose(last.est_w2c[-1], last.opt.matrix())[0]  # last_lm.get_frame_w2c(-1)
        if not lm.tracking_ok:  # re_tracking (Backend.py:54-79): the frontend lost track when this local map began
            n = 2 * int(cfg["frontend"]["num_tracking_iters"])
            first = lm.saved_idxs[0]
            lm.retrack_opt = _pose.PoseOptimizer(w2kf, cfg["cameras"]["frontend_lr"], betas=(0.7, 0.99), left=lm.est_w2c[first])
            self._pose_steps(lm.retrack_opt, lm, [self.rng.choice(lm.saved_idxs) for _ in range(n)])
            w2kf = lm.retrack_opt.matrix()
        lm.opt = _pose.PoseOptimizer(w2kf, cfg["cameras"]["backend_lr"], betas=(0.7, 0.99))
        reps = sorted({0, len(lm.frames) - 2})
        w2c = _ops.compose(lm.est_w2c, w2kf, ia=reps)
        for k, f in enumerate(reps):
            lm.slots.append((self.bank.add(lm.frames[f].gt_depth, w2c[k], group=lmid), f))
        params, lm.params = lm.params, None
        if lmid == 0:
            self.merge_rows.append(localmap.merge_local_map(self.map, params, self.eye, opacity_cap=None))
            tasks = covis.backend_schedule(0, [0], int(be["num_ba_iters"]), int(be["num_covis_submaps"]))
        else:
            transfer = localmap.transfer_matrix(w2kf, lm.ref2f0)
            self.merge_rows.append(localmap.merge_local_map(self.map, params, transfer))
            ids = self.bank.query_covisible(lmid, min(int(be["num_covis_submaps"]), 64))
            tasks = covis.backend_schedule(lmid, ids, int(be["num_ba_iters"]), int(be["num_covis_submaps"]), rng=self.rng)
        self.pruned = 0
        self._run(tasks)

    def final_refine(self):
        """Backend.final_refine (Backend.py:163-172): one map_frames over random (submap, saved frame) draws."""
        iters = int(self.config["backend"]["final_refinement"])
        if iters == -1:
            iters = self.local_maps[-1].frames[-1].time_idx
        self._run_mapping([self.rng.randrange(len(self.local_maps)) for _ in range(iters)])

    def _trajectory_index(self):
        """(submap, frame) of every frame of Localmaps.get_w2cs: frames[:-1] of every map, plus the last frame of the last."""
        idx = [(i, f) for i, lm in enumerate(self.local_maps) for f in range(len(lm.frames) - 1)]
        return idx + [(len(self.local_maps) - 1, len(self.local_maps[-1].frames) - 1)]

    def _gather(self, name, with_transform):
        require(len(self.local_maps) >= 1, "no local map has been handed over")
        offsets, o = [], 0
        for lm in self.local_maps:
            offsets.append(o)
            o += len(lm.frames)
        idx = self._trajectory_index()
        A = torch.cat([getattr(lm, name) for lm in self.local_maps])
        ia = [offsets[i] + f for i, f in idx]
        if not with_transform:
            return _ops.compose(A, ia=ia)
        return _ops.compose(A, self._transforms(), ia=ia, ib=[i for i, _ in idx])

    def trajectory(self):
        """Localmaps.get_w2cs: est_w2c[f] . T[lm] as one [N,4,4] device tensor from one launch."""
        return self._gather("est_w2c", True)

    def gt_trajectory(self):
        """Localmaps.get_gt_w2cs, [N,4,4] on the device."""
        return self._gather("gt_w2c", False)

    def activated_params(self):
        """The global map as render.render takes it: a dict of detached activated tensors."""
        leaves = self.map.render_leaves()
        return OrderedDict((n, t.detach().clone()) for n, t in leaves.items())


def write_trajectory(path, w2cs):
    """World-to-camera poses [N,4,4] as the layout of a Replica traj.txt: camera to world, one row-major 4x4 per line.  The
    inverse is the rigid closed form, in float64 on the host; 17 significant digits, so float32 poses come back exactly."""
    w2cs = torch.as_tensor(w2cs).detach().cpu().double().reshape(-1, 4, 4)
    c2w = torch.zeros_like(w2cs)
    R, t = w2cs[:, :3, :3], w2cs[:, :3, 3]
    c2w[:, :3, :3] = R.transpose(1, 2)
    c2w[:, :3, 3] = -(R.transpose(1, 2) @ t[:, :, None])[:, :, 0]
    c2w[:, 3, 3] = 1.0
    with open(path, "w") as fh:
        for m in c2w.reshape(-1, 16).tolist():
            fh.write(" ".join(repr(v) for v in m) + "\n")


def write_map(path, params):
    """The raw parameters (means3D, opacities, scales, rotations, colors: [P,k] tensors) as the reference's map.ply
    (ply.save_ply)."""
    from . import ply
    host = {n: params[n].detach().cpu().numpy() for n in ("means3D", "opacities", "scales", "rotations", "colors")}
    ply.save_ply(path, host["means3D"], host["opacities"], host["scales"], host["rotations"], rgb=host["colors"])


def write_results(path, evaluation, stamps, data=None, seed=None):
    """results.json: the evaluation (tensors and arrays as lists), the build stamps of the libraries used, the configuration's
    `data` section and the seed."""
    def plain(v):
        if isinstance(v, torch.Tensor):
            return v.detach().cpu().tolist()
        if hasattr(v, "tolist"):
            return v.tolist()
        if isinstance(v, dict):
            return {str(k): plain(x) for k, x in v.items()}
        if isinstance(v, (list, tuple)):
            return [plain(x) for x in v]
        return v if isinstance(v, (bool, int, float, str, type(None))) else str(v)
    with open(path, "w") as fh:
        json.dump(dict(evaluation=plain(evaluation), build=plain(stamps), data=plain(data), seed=seed), fh, indent=1)
        fh.write("\n")


def build_stamps():
    """build_info() of the libraries a run of the driver loads: rasterizer, map, loss, covisibility, frontend, ingest."""
    from . import _covis_lib, _front_lib, _ingest_lib, _lib, _loss_lib, _map_lib
    return OrderedDict((name, mod.build_info()) for name, mod in (("rasterizer", _lib), ("map", _map_lib), ("loss", _loss_lib),
                                                                  ("covis", _covis_lib), ("front", _front_lib), ("ingest", _ingest_lib)))


class SlamResult:
    def __init__(self, frontend, backend, records):
        self.frontend, self.backend, self.records = frontend, backend, records

    def save(self, directory, evaluation=None, data=None, seed=None):
        """Writes results.json (write_results: `evaluation`, or evaluate() when None), traj_est.txt and traj_gt.txt (camera to
        world, the layout of traj.txt) and map.ply (the global map's raw parameters) into `directory`: the tail of the
        reference's scripts/gaus.py.  Returns the evaluation."""
        os.makedirs(directory, exist_ok=True)
        if evaluation is None:
            evaluation = self.evaluate()
        write_results(os.path.join(directory, "results.json"), evaluation, build_stamps(), data, seed)
        write_trajectory(os.path.join(directory, "traj_est.txt"), self.trajectory())
        write_trajectory(os.path.join(directory, "traj_gt.txt"), self.gt_trajectory())
        write_map(os.path.join(directory, "map.ply"), self.backend.map.soa.views)
        return evaluation

    def save_scene(self, directory, config=None):
        """scene_io.save_scene of the run into `directory`: config.json (`config`, or the driver's own configuration when None),
        gaussians.ply (the global map's raw parameters), w2cs.npz.npy and gt_w2cs.npz.npy -- what the reference's save_scence
        leaves under <run>/save for a later evaluation (python -m gaus_slam_amd.nvs)."""
        from . import scene_io
        scene_io.save_scene(directory, self.backend.config if config is None else config, self.backend.map.soa.views, self.trajectory(),
                            self.gt_trajectory())

    def trajectory(self):
        return self.backend.trajectory()

    def gt_trajectory(self):
        return self.backend.gt_trajectory()

    def evaluate(self, **kw):
        """evaluate.evaluate_map on the global map over the saved frames of every submap, at their estimated poses, with the
        ATE of the whole trajectory."""
        from . import evaluate
        b = self.backend
        draws = [(i, f) for i, lm in enumerate(b.local_maps) for f in sorted(lm.saved_idxs)]
        offsets, o = [], 0
        for lm in b.local_maps:
            offsets.append(o)
            o += len(lm.frames)
        settings = b.cameras(torch.cat([lm.est_w2c for lm in b.local_maps]), b._transforms(), ia=[offsets[i] + f for i, f in draws],
                             ib=[i for i, _ in draws])
        frames = [(s, b.local_maps[i].frames[f].gt_color, b.local_maps[i].frames[f].gt_depth) for s, (i, f) in zip(settings, draws)]
        return evaluate.evaluate_map(b.activated_params(), frames, est_w2cs=self.trajectory(), gt_w2cs=self.gt_trajectory(),
                                     **{**_render_kw(b.config), **kw})

    def evaluate_final(self, sequence, **kw):
        """evaluate.evaluate_final on the global map over EVERY frame of `sequence`, the one the run was made from, re-read and
        rendered at its estimated pose: the reference's eval_final, whose numbers are the ones it reports.  The working size,
        the intrinsics, use_sa and the depth normalisation are the run's own; kw: what evaluate_final takes besides (out_dir,
        mesh, mesh_interval, save_renders, lpips, dataset_name, gt_mesh, unseen, prefetch, seed)."""
        from . import evaluate
        b = self.backend
        return evaluate.evaluate_final(b.activated_params(), sequence, (b.W, b.H), self.trajectory(), self.gt_trajectory(),
                                       **{"intrinsics": b.intr, "use_sa": b.use_sa, **_render_kw(b.config), **kw})


def run_slam(sequence, config, seed=0, device="cuda"):
    """The loop of scripts/gaus.py:84-104 over `sequence`: any iterable of (color_u8 [H0,W0,3] uint8, depth [H0,W0] uint16 or
    float32, gt_c2w [4,4]) with the attributes intrinsics (fx, fy, cx, cy at the source size), png_depth_scale and size (W0, H0).
    config['cameras'] height / width give the working size and its intrinsics are filled in from the sequence's, scaled, when
    absent.  Ground-truth poses are taken relative to the first frame.  A sequence with a `distortion` that is not None, or a
    `depth_size` other than its size (gaus_slam_amd/datasets.py), goes through frontend_ops.ingest_ex; every other sequence
    through ingest, as before.  Returns a SlamResult."""
    config = dict(config)
    config["cameras"] = cam = dict(config.get("cameras", {}))
    W0, H0 = sequence.size
    cam.setdefault("width", W0)
    cam.setdefault("height", H0)
    size = (int(cam["width"]), int(cam["height"]))
    if "intrinsics" not in cam:
        fx, fy, cx, cy = _ops.scaled_intrinsics(sequence.intrinsics, (W0, H0), size)
        cam["intrinsics"] = [[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]]
    rng = random.Random(seed)
    frontend, backend = Frontend(config, rng, device), Backend(config, rng, device)
    dev = frontend.device
    records, first_w2c = [], None
    distortion = getattr(sequence, "distortion", None)
    extended = distortion is not None or tuple(getattr(sequence, "depth_size", None) or (W0, H0)) != (W0, H0)
    for time_idx, (color_u8, depth, gt_c2w) in enumerate(sequence):
        if depth.dtype == torch.uint16:  # the same bits under a dtype every copy supports; ingest reads int16 storage as uint16
            depth = depth.view(torch.int16)
        if extended:
            gt_color, gt_depth = _ops.ingest_ex(color_u8.to(dev), depth.to(dev), sequence.png_depth_scale, size, distortion=distortion,
                                                intrinsics=sequence.intrinsics)
        else:
            gt_color, gt_depth = _ops.ingest(color_u8.to(dev), depth.to(dev), sequence.png_depth_scale, size)
        gt_c2w = gt_c2w.to(dev, torch.float32).contiguous()
        if first_w2c is None:
            first_w2c = _ops.compose(gt_c2w, inv_a=True)
        gt_pose = _ops.compose(first_w2c, gt_c2w)[0]  # relative_pose=True of the reference's datasets
        record = frontend.process_frame(time_idx, gt_color, gt_depth, gt_pose)
        if record is not None:
            backend.process_localmap(record)
            records.append(record)
    record = frontend.process_final()
    if record is not None:
        backend.process_localmap(record)
        records.append(record)
    backend.final_refine()
    return SlamResult(frontend, backend, records)
