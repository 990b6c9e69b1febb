"""Denoising-error scan on real images: measure where to set ``--t_switch``.

The shallow backbone of a DuoDiff pair is good enough exactly where its denoising error on real data matches the full backbone's: at the
noisy timesteps.  This tool evaluates the reference's training loss (trainer.py ``_loss_fn``) per timestep on held-out images -- each image
noised to t with a z of its own, the model run on it, the mean squared error against the training target -- for one model or for a
shallow / full pair that sees the same (x0, z, t), and suggests a ``t_switch`` from the paired gap.  The whole scan of a batch is one
device-resident loop (engine.scan_error_loop: dd_scan_error).

    python -m duodiff_amd.switch_scan --config_path configs/uvit_celeba_3.yaml --checkpoint_path s.pth \\
        --config_path_late configs/uvit_celeba.yaml --checkpoint_path_late f.pth --parametrization predict_noise \\
        --images held_out/ --stride 50 --output_folder scan

writes ``scan.npz`` (the per-image errors) and ``scan.json`` (per-timestep means, the paired gap with its standard error, the suggestion).
Images: a folder of PNGs of the model's size (mapped through 2 v - 1) or a ``.npy`` [N, C, S, S] in the model's own space; latent models take
``.npy`` latents, or pixel images with ``--encode_images``.  Per-image seeds are always on: image i is noised under seed ``--seed + i``, so
its numbers depend on the image and its seed, not on the batch it ran in.
"""
import json
import math
from argparse import ArgumentParser
from pathlib import Path

import numpy as np

from .step_plan import SCAN_PARAMETRIZATIONS, scan_rows


def suggest_t_switch(timesteps, e_first, e_late, tolerance, sems=2.0):
    """The largest t_switch the paired errors support, or None.  e_first, e_late: [len(timesteps), N] per-image errors of the first
    (shallow) and the late (full) model on the same (x0, z, t).  Per grid timestep k
        gap_k = mean_i(e_first - e_late) / mean_i(e_late)       sem_k = std_i(e_first - e_late, ddof=1) / sqrt(N) / mean_i(e_late)
    and the timestep is acceptable where gap_k + sems * sem_k <= tolerance.  t_min is the smallest grid timestep with every grid timestep
    >= it acceptable, and the answer is 1000 - t_min: the sampler's switch rule, under which t_switch = 300 runs the first model on
    999 .. 700.  None -- run the late model alone -- where 999 itself is not acceptable (never 0: to the sampler 0 means the first model
    everywhere).  ValueError where 999 is not on the grid.  Pure numpy."""
    return _suggest(timesteps, *gap_statistics(e_first, e_late), tolerance, sems)


def gap_statistics(e_first, e_late):
    """(gap, sem) per timestep of suggest_t_switch, float64; one image: sem = 0"""
    ef, el = np.asarray(e_first, np.float64), np.asarray(e_late, np.float64)
    if ef.shape != el.shape or ef.ndim != 2 or ef.shape[1] < 1:
        raise ValueError("e_first and e_late must both be [timesteps, images]")
    d, base = ef - el, el.mean(axis=1)
    n = ef.shape[1]
    sem = d.std(axis=1, ddof=1) / np.sqrt(n) / base if n > 1 else np.zeros(len(base))
    return d.mean(axis=1) / base, sem


def _suggest(timesteps, gap, sem, tolerance, sems):
    ts = np.asarray(timesteps, np.int64)
    if ts.ndim != 1 or len(ts) != len(gap) or len(set(ts.tolist())) != len(ts):
        raise ValueError("timesteps must be distinct, one per row of the errors")
    if 999 not in ts:
        raise ValueError("the grid must include t = 999: the first model's range starts there")
    ok = dict(zip(ts.tolist(), (np.asarray(gap) + float(sems) * np.asarray(sem) <= float(tolerance)).tolist()))
    t_min = None
    for t in sorted(ok, reverse=True):
        if not ok[t]:
            break
        t_min = t
    return None if t_min is None else 1000 - int(t_min)


def scan_timesteps(timesteps=None, stride=None):
    """--timesteps as given, or --stride N: 999, 999 - N, ... (999 always, 0 only if it is hit)"""
    if (timesteps is None) == (stride is None):
        raise ValueError("give --timesteps or --stride, one of them")
    if stride is not None:
        if stride < 1:
            raise ValueError(f"--stride {stride} must be at least 1")
        return list(range(999, -1, -int(stride)))
    ts = [int(t) for t in timesteps]
    if not ts or any(not 0 <= t <= 999 for t in ts):
        raise ValueError("--timesteps must lie in [0, 999]")
    if len(set(ts)) != len(ts):
        raise ValueError("--timesteps holds a timestep twice")
    return ts


def get_args(argv=None):
    p = ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--seed", type=int, default=0, help="image i is noised under seed --seed + i")
    p.add_argument("--config_path", type=str, required=True, help="Path to yaml config file")
    p.add_argument("--checkpoint_path", type=str, required=True, help="Path to checkpoint of the model")
    p.add_argument("--config_path_late", type=str, default=None, help="yaml config of the late (full) model: a paired scan")
    p.add_argument("--checkpoint_path_late", type=str, default=None, help="checkpoint of the late (full) model")
    p.add_argument("--autoencoder_checkpoint_path", type=str, default=None, help="overrides config['autoencoder']['autoencoder_checkpoint_path']")
    p.add_argument("--parametrization", type=str, required=True, choices=list(SCAN_PARAMETRIZATIONS))
    p.add_argument("--images", type=str, required=True, help="a folder of PNGs of the model's size, or a .npy [N, C, S, S] in the model's space")
    p.add_argument("--encode_images", action="store_true", help="latent models: --images are pixels ([N, 3, 8S, 8S] in [-1, 1], or PNGs); they go through the KL-VAE encoder")
    p.add_argument("--encode_mean", action="store_true", help="with --encode_images: the posterior's mode instead of a sample")
    p.add_argument("--class_label", type=int, default=None, help="every image gets this class label")
    p.add_argument("--labels", type=str, default=None, help=".npy of one integer label per image")
    p.add_argument("--timesteps", type=int, nargs="+", default=None, metavar="T")
    p.add_argument("--stride", type=int, default=None, metavar="N", help="the grid 999, 999 - N, ...")
    p.add_argument("--repeats", type=int, default=1, metavar="R", help="R scans with fresh noise (Philox counters r * len(grid) + k), averaged per image")
    p.add_argument("--tolerance", type=float, default=0.02, help="largest acceptable relative gap of the first model's error over the late model's")
    p.add_argument("--sems", type=float, default=2.0, help="standard errors of the gap added before it is compared with --tolerance")
    p.add_argument("--batch_size", type=int, default=128)
    p.add_argument("--output_folder", type=str, required=True)
    p.add_argument("--precision", choices=["bf16", "fp32"], default="bf16")
    p.add_argument("--no_graph", action="store_true", help="launch kernels eagerly instead of hipGraph replay")
    return p.parse_args(argv)


def validate(args, config, config_late=None):
    """Every option check that needs no image and no GPU, before the first model is built: ValueError on a bad combination.  Returns the grid."""
    from .config import ModelParams
    grid = scan_timesteps(args.timesteps, args.stride)
    if args.seed < 0:
        raise ValueError("--seed must not be negative: image i is noised under seed --seed + i")
    if args.repeats < 1:
        raise ValueError(f"--repeats {args.repeats} must be at least 1")
    if args.batch_size < 1:
        raise ValueError(f"--batch_size {args.batch_size} must be at least 1")
    if not (math.isfinite(args.tolerance) and args.tolerance >= 0):
        raise ValueError(f"--tolerance {args.tolerance} must be finite and not negative")
    if not (math.isfinite(args.sems) and args.sems >= 0):
        raise ValueError(f"--sems {args.sems} must be finite and not negative")
    if (args.config_path_late is None) != (args.checkpoint_path_late is None):
        raise ValueError("--config_path_late and --checkpoint_path_late go together")
    if args.class_label is not None and args.labels is not None:
        raise ValueError("--class_label and --labels are exclusive")
    mp = ModelParams.from_dict(config)
    latent = "autoencoder" in config
    for name, cfg in (("--config_path", config), ("--config_path_late", config_late)):
        if cfg is None:
            continue
        m = ModelParams.from_dict(cfg)
        if (m.img_size, m.in_chans) != (mp.img_size, mp.in_chans) or ("autoencoder" in cfg) != latent:
            raise ValueError("the two models disagree on the image shape (img_size, in_chans, autoencoder)")
        labelled = args.class_label is not None or args.labels is not None
        if m.num_classes > 0 and not labelled:
            raise ValueError(f"{name} is class-conditional: give --class_label or --labels")
        if m.num_classes <= 0 and labelled:
            raise ValueError(f"--class_label / --labels need class-conditional configs; {name} has none")
        if args.class_label is not None and not 0 <= args.class_label < m.num_classes:
            raise ValueError(f"--class_label {args.class_label} outside [0, {m.num_classes}) of {name}")
    if config_late is not None and 999 not in grid:
        raise ValueError("a paired scan suggests a t_switch: the grid must include t = 999")
    if args.encode_images:
        if not latent:
            raise ValueError("--encode_images needs a latent model (a config with an autoencoder block)")
        if mp.in_chans != 4 or mp.img_size % 8 or mp.img_size > 32:
            raise ValueError("--encode_images: the KL-VAE encoder gives 4-channel latents of a size that is a multiple of 8, at most 32")
    elif args.encode_mean:
        raise ValueError("--encode_mean goes with --encode_images")
    path = Path(args.images)
    if path.suffix.lower() != ".npy" and not path.is_dir():
        raise ValueError(f"--images {args.images}: a folder of PNGs or a .npy file")
    if path.is_dir() and latent and not args.encode_images:
        raise ValueError("--images: a latent model takes .npy latents, or pixel images with --encode_images")
    if path.is_dir() and not latent and mp.in_chans != 3:
        raise ValueError(f"--images: PNGs need an in_chans = 3 config, this one has in_chans = {mp.in_chans}")
    return grid


def load_images(args, mp):
    """--images -> float32 [N, C, S, S] in [-1, 1] (PNGs) or as stored (.npy); the size must be the model's (8 x under --encode_images)"""
    path = Path(args.images)
    if path.is_dir():
        from .evaluation import read_samples
        x = 2.0 * read_samples(path).numpy().astype(np.float32) - 1.0
    else:
        x = np.asarray(np.load(path), np.float32)
    chans, size = (3, 8 * mp.img_size) if args.encode_images else (mp.in_chans, mp.img_size)
    if x.ndim != 4 or x.shape[0] < 1 or x.shape[1:] != (chans, size, size):
        raise ValueError(f"--images: shape {list(x.shape)} does not match [N, {chans}, {size}, {size}] (images are not resized)")
    if not np.isfinite(x).all():
        raise ValueError("--images: non-finite values")
    return np.ascontiguousarray(x)


def load_labels(args, n, num_classes):
    if args.class_label is not None:
        return np.full(n, int(args.class_label), np.int64)
    if args.labels is None:
        return None
    y = np.load(args.labels)
    if y.shape != (n,) or not np.issubdtype(y.dtype, np.integer):
        raise ValueError(f"--labels: need {n} integers, one per image")
    if y.min() < 0 or y.max() >= num_classes:
        raise ValueError(f"--labels outside [0, {num_classes})")
    return y.astype(np.int64)


def scan(models, x0, y, rows, seed, repeats, batch_size, use_graph=True):
    """The errors of every model of `models` (engine Models) on x0 [N, C, S, S] (numpy): [len(models), repeats, len(grid), N] float32.  The
    images run in batches of batch_size; image i under seed + i whatever its batch; repeat r draws with Philox counters r n + k.  Every
    model sees the same (x0, z, t)."""
    import torch
    from .engine import scan_error_loop
    n, N = len(rows["t"]), len(x0)
    out = np.zeros((len(models), repeats, n, N), np.float32)
    ctx = models[0].ctx
    for i0 in range(0, N, batch_size):
        i1 = min(i0 + batch_size, N)
        xb = torch.from_numpy(x0[i0:i1]).cuda().contiguous()
        yb = None if y is None else torch.from_numpy(y[i0:i1]).cuda()
        with ctx.image_seeds([int(seed) + i for i in range(i0, i1)]):
            for r in range(repeats):
                for j, m in enumerate(models):
                    out[j, r, :, i0:i1] = scan_error_loop(ctx, m, xb, rows, y=yb, counter_base=r * n, use_graph=use_graph).cpu().numpy()
    return out


def summarize(args, grid, err, names):
    """scan.json: per-timestep means of each model and, for a pair, gap, sem, what is acceptable and the suggestion"""
    per_image = err.astype(np.float64).mean(axis=1)                      # [models, n, N]: the repeats averaged per image
    out = {"parametrization": args.parametrization, "timesteps": [int(t) for t in grid], "images": int(err.shape[-1]), "repeats": int(args.repeats),
           "seed": int(args.seed), "precision": args.precision,
           "models": {name: {"mean_error": per_image[j].mean(axis=1).tolist()} for j, name in enumerate(names)}}
    if len(names) == 2:
        gap, sem = gap_statistics(per_image[0], per_image[1])
        t_switch = _suggest(grid, gap, sem, args.tolerance, args.sems)
        out.update(gap=gap.tolist(), sem=sem.tolist(), acceptable=(gap + args.sems * sem <= args.tolerance).tolist(),
                   tolerance=float(args.tolerance), sems=float(args.sems), t_switch=t_switch,
                   advice=f"--t_switch {t_switch}" if t_switch is not None else "run the late model alone (the first model misses the tolerance at t = 999)")
    return out


def main(argv=None):
    import torch
    from .config import ModelParams, load_config
    from .sampler import build_model, load_autoencoder
    args = get_args(argv)
    config = load_config(args.config_path)
    config_late = load_config(args.config_path_late) if args.config_path_late else None
    grid = validate(args, config, config_late)
    mp = ModelParams.from_dict(config)
    x0 = load_images(args, mp)
    y = load_labels(args, len(x0), mp.num_classes)
    out = Path(args.output_folder)
    out.mkdir(parents=True, exist_ok=True)
    bs = min(args.batch_size, len(x0))
    models = [build_model(config, args.checkpoint_path, args.precision, bs)[0]]
    names = ["first"]
    if config_late is not None:
        models.append(build_model(config_late, args.checkpoint_path_late, args.precision, bs)[0])
        names.append("late")
    if args.encode_images:
        print("Encode the images...")
        ae = load_autoencoder(args, config, models[0].device)
        x0 = np.concatenate([ae.encode(torch.from_numpy(x0[i:i + 1]), generator=torch.Generator().manual_seed(int(args.seed) + i),
                                       sample=not args.encode_mean).cpu().numpy() for i in range(len(x0))])
    rows = scan_rows(grid, args.parametrization)
    err = scan([m.engine_model(bs) for m in models], x0, y, rows, args.seed, args.repeats, bs, use_graph=not args.no_graph)
    np.savez(out / "scan.npz", timesteps=np.asarray(grid, np.int64), image_seeds=np.arange(len(x0), dtype=np.int64) + int(args.seed),
             **{f"err_{name}": err[j] for j, name in enumerate(names)})
    summary = summarize(args, grid, err, names)
    (out / "scan.json").write_text(json.dumps(summary, indent=1) + "\n")
    for k, t in enumerate(grid):
        line = f"t = {t:3d}  " + "  ".join(f"{name} {summary['models'][name]['mean_error'][k]:.6f}" for name in names)
        if len(names) == 2:
            line += f"  gap {summary['gap'][k]:+.4f} +- {summary['sem'][k]:.4f}{'' if summary['acceptable'][k] else '  *'}"
        print(line)
    if len(names) == 2:
        print(summary["advice"])


if __name__ == "__main__":
    main()
