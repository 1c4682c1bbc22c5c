"""Checkpoints of train_step.Trainer: one `torch.save` file that the
reference's trainer reads (simple_trainer.py:734-747 writes, :1055-1064 reads
`ckpt["step"]` and `ckpt["splats"]`) and that resumes a run of this trainer
exactly.

    "step"         index of the last completed step
    "splats"       name -> tensor under the reference ParameterDict's names
                   (means scales quats opacities sh0 shN; app_opt: features,
                   colors instead of sh0 / shN)
    "pose_adjust"  {"embeds.weight": [n_img, 9]}            with pose_opt
    "app_module"   AppearanceOptimizer.state_dict()         with app_opt
    "gsplat_hip"   everything else the next step reads that is neither a
                   constructor argument nor the dataset (the reference ignores
                   the key): format version, the Adam moments and step counts,
                   the bilateral grids, the strategy statistics and refine log,
                   the generator state and noise key, the pose-noise table, the
                   tuned forward variant and a fingerprint of the configuration

The file holds only CPU tensors, numbers, strings, lists and dicts, so it loads
with `torch.load(weights_only=True)`.  Restoring goes the way Trainer.refine
replaces its tensors (new Parameters, _load_moments, _register_hooks,
_param_gen += 1: a captured step re-captures at its next step); tensors whose
shape the constructor fixed are copied in place by their owners, Trainer.sides
(losses.SideOptimizer names its tables and moments; none is named here).
"""

import dataclasses

import torch

FORMAT_VERSION = 1
SPLIT_KEYS = ("split_div", "split_threshold", "split_launch", "_split_tuned", "term_ratio",
              "max_tile_first")


def refuse(tr, what):
    from .train_step import _refuse
    _refuse("checkpoint", {"gaussian_shard": tr.gshard, "sharded_optimizer": bool(tr.sharded),
                           "world_size": tr.world_size != 1}, name=what)


def _plain(v):
    """A config value as a number, string, bool, None or list of those."""
    if isinstance(v, (tuple, list)):
        return [_plain(x) for x in v]
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return repr(v)


def fingerprint(tr) -> dict:
    """What a resumed trainer must have been constructed with, as a flat dict
    of plain values."""
    fp = {"model": tr.model, "sh_degree": int(tr.sh_degree), "fused": bool(tr.fused),
          "n_images": int(len(tr.viewmats)), "width": int(tr.width), "height": int(tr.height),
          "params": list(tr.params),
          "strategy": None if tr.strategy is None else type(tr.strategy).__name__}
    for k in ("bilateral_grid", "pose_opt", "depth_loss", "app_opt", "normal_loss", "dist_loss",
              "packed", "sparse_grad", "visible_adam"):
        fp[k] = bool(getattr(tr, k))
    for k in ("pose_noise", "opacity_reg", "scale_reg", "ssim_lambda", "scene_scale",
              "rasterize_mode", "max_steps", "sh_degree_interval"):
        fp[k] = _plain(getattr(tr, k))
    if tr.bilateral_grid:
        fp["bilateral_grid_shape"] = _plain(tr.bilateral_grid_shape)
    # only when on: the fingerprints of trainers without them, and of files
    # written before the options existed, are unchanged
    if tr.masks is not None:
        fp["masks"] = True
    if tr.random_bkgd:
        fp["random_bkgd"] = True
    if tr.strategy is not None:
        for k, v in dataclasses.asdict(tr.strategy).items():
            fp["strategy." + k] = _plain(v)
    return fp


def _adam_step(tr) -> int:
    opt = tr.opt
    if hasattr(opt, "step_count"):
        return int(opt.step_count)
    st = next(iter(opt.state.values()), {}).get("step", 0)
    return int(st.item()) if torch.is_tensor(st) else int(st)


def _set_adam_step(tr, moments, step):
    opt = tr.opt
    if hasattr(opt, "step_count"):
        opt.step_count = int(step)
        return
    sparse = isinstance(opt, torch.optim.SparseAdam)
    for k, p in tr.params.items():
        opt.state[p] = {"step": int(step) if sparse else torch.tensor(float(step)),
                        "exp_avg": moments[k][0], "exp_avg_sq": moments[k][1]}


def _cpu(t):
    if isinstance(t, dict):
        return {k: _cpu(v) for k, v in t.items()}
    return t.detach().to("cpu", copy=True).contiguous()


def state(tr, step) -> dict:
    """The checkpoint of `tr` after step `step` as a dict (module docstring)."""
    tr.sync()
    out = {"step": int(step), "splats": {k: _cpu(p) for k, p in tr.params.items()}}
    tables = [so.checkpoint_tables() for so in tr.sides]
    for ref, _ in tables:
        out.update(_cpu(ref))
    gs = {"format": FORMAT_VERSION, "fingerprint": fingerprint(tr),
          "moments": {k: [_cpu(m), _cpu(v)] for k, (m, v) in tr.moments().items()},
          "adam_step": _adam_step(tr),
          "side_steps": {so.name: int(so.step_count) for so in tr.side_opts},
          "grad2d": _cpu(tr.grad2d), "count": _cpu(tr.count),
          "radii2d": None if tr.radii2d is None else _cpu(tr.radii2d),
          "refine_log": [[int(x) for x in row] for row in tr.refine_log],
          "rng": _cpu(tr.rng.get_state()), "noise_seed": str(int(tr._noise_seed)),
          "split": {k: _plain(getattr(tr, k, None)) for k in SPLIT_KEYS}}
    for _, own in tables:
        gs.update(_cpu(own))
    out["gsplat_hip"] = gs
    return out


def save(tr, path, step):
    refuse(tr, "save_checkpoint (checkpoint)")
    torch.save(state(tr, step), path)


def _check_fingerprint(tr, saved):
    mine = fingerprint(tr)
    diff = [f"{k}: checkpoint {saved.get(k)!r}, trainer {mine.get(k)!r}"
            for k in sorted(set(mine) | set(saved)) if mine.get(k) != saved.get(k)]
    if diff:
        raise ValueError("load_checkpoint: the trainer's configuration differs from the "
                         "checkpoint's in " + "; ".join(diff))


def _install(tr, params, moments, step):
    """New parameter tensors and moments, the way refine() installs them."""
    dev = tr.device
    tr.sync()
    tr.last_meta = None
    tr.params = {k: torch.nn.Parameter(v.to(dev, torch.float32).contiguous())
                 for k, v in params.items()}
    moments = {k: [m.to(dev, torch.float32).contiguous(), v.to(dev, torch.float32).contiguous()]
               for k, (m, v) in moments.items()}
    tr._load_moments(moments)
    _set_adam_step(tr, moments, step)
    tr._register_hooks()
    tr._param_gen += 1  # a captured step re-captures


def _fresh_statistics(tr):
    n = tr.params["means"].shape[0]
    tr.grad2d = torch.zeros(n, device=tr.device)
    tr.count = torch.zeros(n, device=tr.device)
    if tr.radii2d is not None:
        tr.radii2d = torch.zeros(n, device=tr.device)
    tr.refine_log = []


def _check_splats(tr, splats, who):
    names = list(tr.params)
    missing = [k for k in names if k not in splats]
    if missing:
        raise ValueError(f"{who}: no {missing} among the splats {sorted(splats)}; the trainer "
                         f"holds {names}")
    n = splats["means"].shape[0]
    for k in names:
        want = (n,) + tuple(tr.params[k].shape[1:])
        if tuple(splats[k].shape) != want:
            raise ValueError(f"{who}: {k} is {list(splats[k].shape)}, the trainer's is "
                             f"{list(want)} for {n} Gaussians")
    return names


def load_splats(tr, splats):
    """The Gaussians of `splats` (name -> tensor, e.g. load_ply's or
    PngCompression.decompress's) as the trainer's parameters: zero moments and
    step count, fresh statistics (the evaluation path; a start for fine-tuning).
    The side optimizers keep their tables, moments and step counts."""
    refuse(tr, "load_splats (checkpoint)")
    names = _check_splats(tr, splats, "load_splats")
    params = {k: splats[k].detach() for k in names}
    zeros = {k: [torch.zeros_like(v, dtype=torch.float32),
                 torch.zeros_like(v, dtype=torch.float32)] for k, v in params.items()}
    _install(tr, params, zeros, 0)
    _fresh_statistics(tr)


@torch.no_grad()
def load(tr, paths, resume=True):
    """Trainer.load_checkpoint: returns the checkpoint's step."""
    refuse(tr, "load_checkpoint (checkpoint)")
    many = isinstance(paths, (list, tuple))
    files = list(paths) if many else [paths]
    if not files:
        raise ValueError("load_checkpoint: no file given")
    cks = [torch.load(f, map_location="cpu", weights_only=True) for f in files]
    step = int(cks[0]["step"])
    if many or not resume or "gsplat_hip" not in cks[0]:
        if resume and not many:
            raise ValueError(f"load_checkpoint: {files[0]} has no 'gsplat_hip' block (a "
                             "checkpoint of the reference trainer): it cannot resume a run; "
                             "pass resume=False to load its Gaussians")
        # simple_trainer.py:1061-1062: the files' Gaussians concatenated
        splats = {k: torch.cat([ck["splats"][k] for ck in cks]) for k in cks[0]["splats"]}
        load_splats(tr, splats)
        for so in tr.sides:  # pose_adjust / app_module of the first: the reference's keys alone
            so.load_checkpoint_tables(cks[0], {}, reset=True)
        return step
    ck = cks[0]
    gs = ck["gsplat_hip"]
    if gs.get("format") != FORMAT_VERSION:
        raise ValueError(f"load_checkpoint: format {gs.get('format')!r} of {files[0]}, this "
                         f"version reads {FORMAT_VERSION}")
    _check_fingerprint(tr, gs["fingerprint"])
    names = _check_splats(tr, ck["splats"], "load_checkpoint")
    dev = tr.device
    _install(tr, {k: ck["splats"][k] for k in names}, gs["moments"], gs["adam_step"])
    for so in tr.sides:  # (their moments went in with the Gaussians': Trainer._load_moments)
        so.load_checkpoint_tables(ck, gs)
    for so in tr.side_opts:
        so.step_count = int(gs["side_steps"][so.name])
    tr.grad2d = gs["grad2d"].to(dev)
    tr.count = gs["count"].to(dev)
    tr.radii2d = None if gs["radii2d"] is None else gs["radii2d"].to(dev)
    tr.refine_log = [tuple(row) for row in gs["refine_log"]]
    tr.rng.set_state(gs["rng"])
    tr._noise_seed = int(gs["noise_seed"])
    for k, v in gs["split"].items():
        if v is not None or k in ("split_div", "split_threshold"):
            setattr(tr, k, v)
    return step


@torch.no_grad()
def save_ply(tr, path, sh_degree=None, transform=None):
    """Trainer.save_ply: the parameters as a PLY file (io.save_ply); app_opt:
    the colours baked as simple_trainer.py:753-763 does.  `transform`: a [4,4]
    similarity the Gaussians are moved by first (transform.transform_splats);
    the baked colours of app_opt are taken before the move and keep their
    values."""
    from .io import save_ply as _save_ply
    refuse(tr, "save_ply (checkpoint)")
    p = {k: v.data for k, v in tr.synced_params().items()}
    if not tr.app_opt:
        if transform is not None:
            from .transform import transform_splats
            p = transform_splats(p, transform)
        return _save_ply(p, path)
    from .appearance import appearance_colors
    deg = tr.sh_degree if sh_degree is None else int(sh_degree)
    zeros = torch.zeros_like(p["means"])
    colors = appearance_colors(p["features"], p["colors"], None, zeros,
                               torch.zeros(1, 3, device=zeros.device), tr.app.head, deg)[0]
    geom = {k: p[k] for k in ("means", "scales", "quats", "opacities")}
    if transform is not None:
        from .transform import transform_splats
        geom = transform_splats(geom, transform)
    return _save_ply(geom, path, colors)
