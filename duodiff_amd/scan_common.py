"""What the two scan tools share (``switch_scan``: a plain model or a shallow / full pair; ``threshold_scan``: an early-exit model): the
timestep grid, the paired gap statistics, the images and labels, the options both take with their checks, and the batch loop."""
import math
from pathlib import Path

import numpy as np


def gap_statistics(e_first, e_late):
    """(gap, sem) per timestep of switch_scan.suggest_t_switch, float64; one image: sem = 0"""
    ef, el = np.asarray(e_first, np.float64), np.asarray(e_late, np.float64)
    if ef.shape != el.shape or ef.ndim != 2 or ef.shape[1] < 1:
        raise ValueError("e_first and e_late must both be [timesteps, images]")
    d, base = ef - el, el.mean(axis=1)
    n = ef.shape[1]
    sem = d.std(axis=1, ddof=1) / np.sqrt(n) / base if n > 1 else np.zeros(len(base))
    return d.mean(axis=1) / base, sem


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


def add_scan_options(p, config_help, checkpoint_help, tolerance_help, own):
    """The options both tools take, in the order --help lists them; own(p, after) adds the tool's own behind the shared option `after`
    ("checkpoint_path", "images", "stride")."""
    p.add_argument("--seed", type=int, default=0, help="image i is noised under seed --seed + i")
    p.add_argument("--config_path", type=str, required=True, help=config_help)
    p.add_argument("--checkpoint_path", type=str, required=True, help=checkpoint_help)
    own(p, "checkpoint_path")
    p.add_argument("--images", type=str, required=True, help="a folder of PNGs of the model's size, or a .npy [N, C, S, S] in the model's space")
    own(p, "images")
    p.add_argument("--class_label", type=int, default=None, help="every image gets this class label")
    p.add_argument("--labels", type=str, default=None, help=".npy of one integer label per image")
    p.add_argument("--timesteps", type=int, nargs="+", default=None, metavar="T")
    p.add_argument("--stride", type=int, default=None, metavar="N", help="the grid 999, 999 - N, ...")
    own(p, "stride")
    p.add_argument("--repeats", type=int, default=1, metavar="R", help="R scans with fresh noise (Philox counters r * len(grid) + k), averaged per image")
    p.add_argument("--tolerance", type=float, default=0.02, help=tolerance_help)
    p.add_argument("--sems", type=float, default=2.0, help="standard errors of the gap added before it is compared with --tolerance")
    p.add_argument("--batch_size", type=int, default=128)
    p.add_argument("--output_folder", type=str, required=True)
    p.add_argument("--precision", choices=["bf16", "fp32"], default="bf16")
    p.add_argument("--no_graph", action="store_true", help="launch kernels eagerly instead of hipGraph replay")


def check_numbers(args):
    """--seed, --repeats, --batch_size, --tolerance, --sems"""
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


def check_label_options(args):
    if args.class_label is not None and args.labels is not None:
        raise ValueError("--class_label and --labels are exclusive")


def check_labels(args, num_classes, name=None):
    """--class_label / --labels against a config's num_classes.  name: the config's option, in the tool that takes two configs."""
    labelled = args.class_label is not None or args.labels is not None
    if num_classes > 0 and not labelled:
        raise ValueError(f"{name or '--config_path'} is class-conditional: give --class_label or --labels")
    if num_classes <= 0 and labelled:
        raise ValueError("--class_label / --labels need " + (f"class-conditional configs; {name} has none" if name else "a class-conditional config"))
    if args.class_label is not None and not 0 <= args.class_label < num_classes:
        raise ValueError(f"--class_label {args.class_label} outside [0, {num_classes})" + (f" of {name}" if name else ""))


def check_images_path(images, in_chans, latent=False, encode=False):
    """--images before anything is read: a .npy or a folder, and a folder only where its PNGs can be the model's input"""
    path = Path(images)
    if path.suffix.lower() != ".npy" and not path.is_dir():
        raise ValueError(f"--images {images}: a folder of PNGs or a .npy file")
    if path.is_dir() and latent and not encode:
        raise ValueError("--images: a latent model takes .npy latents, or pixel images with --encode_images")
    if path.is_dir() and not latent and in_chans != 3:
        raise ValueError(f"--images: PNGs need an in_chans = 3 config, this one has in_chans = {in_chans}")


def load_images(images, chans, size):
    """--images -> float32 [N, chans, size, size] in [-1, 1] (PNGs) or as stored (.npy); images are not resized"""
    path = Path(images)
    if path.is_dir():
        from .evaluation import read_samples
        x = 2.0 * read_samples(path).numpy().astype(np.float32) - 1.0
    else:
        x = np.asarray(np.load(path), np.float32)
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


def batches(ctx, x0, y, seed, batch_size):
    """x0 [N, C, S, S] and y (or None), numpy, in batches of batch_size: yields (x, y, slice) with x and y on the device and the slice the
    batch's images, inside ctx.image_seeds of those images -- image i under seed + i whatever its batch."""
    import torch
    for i0 in range(0, len(x0), batch_size):
        i1 = min(i0 + batch_size, len(x0))
        xb = torch.from_numpy(x0[i0:i1]).cuda().contiguous()
        yb = None if y is None else torch.from_numpy(y[i0:i1]).cuda()
        with ctx.image_seeds([int(seed) + i for i in range(i0, i1)]):
            yield xb, yb, slice(i0, i1)
