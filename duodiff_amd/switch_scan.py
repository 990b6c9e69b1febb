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
from argparse import ArgumentParser
from pathlib import Path

import numpy as np

from .scan_common import (add_scan_options, batches, check_images_path, check_label_options, check_labels, check_numbers, gap_statistics,
                          load_images, load_labels, scan_timesteps)
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


def get_args(argv=None):
    p = ArgumentParser(description=__doc__.split("\n\n")[0])
    def own(p, after):
        if after == "checkpoint_path":
            p.add_argument("--config_path_late", type=str, default=None, help="yaml config of the late (full) model: a paired scan")
            p.add_argument("--checkpoint_path_late", type=str, default=None, help="checkpoint of the late (full) model")
            p.add_argument("--autoencoder_checkpoint_path", type=str, default=None, help="overrides config['autoencoder']['autoencoder_checkpoint_path']")
            p.add_argument("--parametrization", type=str, required=True, choices=list(SCAN_PARAMETRIZATIONS))
        if after == "images":
            p.add_argument("--encode_images", action="store_true", help="latent models: --images are pixels ([N, 3, 8S, 8S] in [-1, 1], or PNGs); they go through the KL-VAE encoder")
            p.add_argument("--encode_mean", action="store_true", help="with --encode_images: the posterior's mode instead of a sample")
    add_scan_options(p, "Path to yaml config file", "Path to checkpoint of the model",
                     "largest acceptable relative gap of the first model's error over the late model's", own)
    return p.parse_args(argv)


def validate(args, config, config_late=None):
    """Every option check that needs no image and no GPU, before the first model is built: ValueError on a bad combination.  Returns the grid."""
    from .config import ModelParams
    grid = scan_timesteps(args.timesteps, args.stride)
    check_numbers(args)
    if (args.config_path_late is None) != (args.checkpoint_path_late is None):
        raise ValueError("--config_path_late and --checkpoint_path_late go together")
    check_label_options(args)
    mp = ModelParams.from_dict(config)
    latent = "autoencoder" in config
    for name, cfg in (("--config_path", config), ("--config_path_late", config_late)):
        if cfg is None:
            continue
        m = ModelParams.from_dict(cfg)
        if (m.img_size, m.in_chans) != (mp.img_size, mp.in_chans) or ("autoencoder" in cfg) != latent:
            raise ValueError("the two models disagree on the image shape (img_size, in_chans, autoencoder)")
        check_labels(args, m.num_classes, name)
    if config_late is not None and 999 not in grid:
        raise ValueError("a paired scan suggests a t_switch: the grid must include t = 999")
    if args.encode_images:
        if not latent:
            raise ValueError("--encode_images needs a latent model (a config with an autoencoder block)")
        if mp.in_chans != 4 or mp.img_size % 8 or mp.img_size > 32:
            raise ValueError("--encode_images: the KL-VAE encoder gives 4-channel latents of a size that is a multiple of 8, at most 32")
    elif args.encode_mean:
        raise ValueError("--encode_mean goes with --encode_images")
    check_images_path(args.images, mp.in_chans, latent, args.encode_images)
    return grid


def scan(models, x0, y, rows, seed, repeats, batch_size, use_graph=True):
    """The errors of every model of `models` (engine Models) on x0 [N, C, S, S] (numpy): [len(models), repeats, len(grid), N] float32.  The
    images run in batches of batch_size; image i under seed + i whatever its batch; repeat r draws with Philox counters r n + k.  Every
    model sees the same (x0, z, t)."""
    from .engine import scan_error_loop
    n, N = len(rows["t"]), len(x0)
    out = np.zeros((len(models), repeats, n, N), np.float32)
    ctx = models[0].ctx
    for xb, yb, at in batches(ctx, x0, y, seed, batch_size):
        for r in range(repeats):
            for j, m in enumerate(models):
                out[j, r, :, at] = scan_error_loop(ctx, m, xb, rows, y=yb, counter_base=r * n, use_graph=use_graph).cpu().numpy()
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
    x0 = load_images(args.images, *((3, 8 * mp.img_size) if args.encode_images else (mp.in_chans, mp.img_size)))
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
