"""Early-exit scan on real images: measure what a ``--threshold`` of the early-exit sampler costs.

The early-exit sampler (``python -m duodiff_amd.eesampler``) leaves the backbone at the first layer whose probe predicts an error at or
below one global ``--threshold``.  This tool evaluates, per timestep on held-out images and from ONE forward each, every exit's error
against the training target (the reference's ``L_n_t``, trainer.py:358-398), the probes' own training target ``mean(tanh|d|)`` and what
the probes predicted; replays the sampler's exit rule on the recorded predictions for a list of candidate thresholds; and says which
threshold keeps the realised error within ``--tolerance`` of the backbone's at every timestep -- or to run the backbone alone.  The whole
scan of a batch is one device-resident loop (engine.scan_exits_loop: dd_scan_error_early_exit).

    python -m duodiff_amd.threshold_scan --config_path configs/deediff_celeba.yaml --checkpoint_path ee.pth \\
        --parametrization predict_noise --images held_out/ --stride 50 --output_folder scan

writes ``exits.npz`` (timesteps, image_seeds, mse, target, predicted, each with a leading repeats axis) and ``exits.json`` (per-timestep
per-exit means, probe calibration, the per-candidate table, the suggestion).  Images, labels and the grid are ``switch_scan``'s; per-image
seeds are always on.
"""
import json
import math
from argparse import ArgumentParser
from pathlib import Path

import numpy as np

from .scan_common import (add_scan_options, batches, check_images_path, check_label_options, check_labels, check_numbers, gap_statistics,
                          load_images, load_labels, scan_timesteps)

PARAMETRIZATIONS = ("predict_noise", "predict_original")       # the two the reference's trainer allows for the early-exit model
F32 = np.float32
TANH_CLAMP = F32(10.0)


def tanh_abs_f32(d):
    """The numpy-float32 mirror of scan_tanh_abs (csrc/step_update.h), bit for bit: tanh|d| from individually rounded float32 + and x, two
    correctly rounded divisions, fabs and min.  d: any array; returns float32 of its shape, in [0, 1]."""
    a = np.fmin(np.abs(np.asarray(d, F32)), TANH_CLAMP)
    h = F32(0.5) * a
    s = h * h
    p = ((s + F32(378.0)) * s + F32(17325.0)) * s + F32(135135.0)
    q = ((F32(28.0) * s + F32(3150.0)) * s + F32(62370.0)) * s + F32(135135.0)
    t = (h * p) / q
    return np.fmin((t + t) / (t * t + F32(1.0)), F32(1.0))


def simulate_exits(pred, threshold):
    """The early-exit sampler's rule (eesampler.py:62-68; dd_early_exit_select) on recorded predictions pred [n, depth, N] (float32):
    a zero row is appended, the comparison is float32 pred <= float32(threshold), the first True wins and an all-False column gives 0.
    Returns the exit index [n, N] (depth: the backbone).  Pure numpy."""
    p = np.asarray(pred, F32)
    if p.ndim != 3:
        raise ValueError("pred must be [timesteps, depth, images]")
    c = np.concatenate([p, np.zeros_like(p[:, :1])], axis=1)
    return np.argmax((c <= F32(threshold)).astype(np.int32), axis=1)


def threshold_statistics(mse, idx):
    """What the exits idx [n, N] (simulate_exits) cost on mse [n, depth + 1, N]: the realised error mse[k, idx[k, i], i] against the
    backbone's mse[k, depth, i], paired per image.  Returns (gap [n], sem [n], blocks): gap and sem as scan_common.gap_statistics,
    blocks = mean(idx) / depth -- exit l reads the input of block l, so it costs l blocks, the backbone depth.  With a leading repeats
    axis on both (mse [R, n, depth + 1, N], idx [R, n, N]: the rule replayed per repeat, as the sampler decides on one draw) the realised
    and the backbone's error are averaged per image over the repeats first.  Pure numpy."""
    m, ix = np.asarray(mse, np.float64), np.asarray(idx, np.int64)
    if m.ndim == 3:
        m, ix = m[None], ix[None] if ix.ndim == 2 else ix
    if m.ndim != 4 or m.shape[2] < 2 or ix.shape != (m.shape[0], m.shape[1], m.shape[3]) or ix.min() < 0 or ix.max() >= m.shape[2]:
        raise ValueError("mse must be [(repeats,) timesteps, depth + 1, images] and idx [(repeats,) timesteps, images] exit indices")
    depth = m.shape[2] - 1
    realised = np.take_along_axis(m, ix[:, :, None, :], axis=2)[:, :, 0, :].mean(axis=0)
    gap, sem = gap_statistics(realised, m[:, :, depth, :].mean(axis=0))
    return gap, sem, float(ix.mean() / depth)


def suggest_threshold(thresholds, gaps, sems_k, tolerance, sems=2.0):
    """The largest candidate of `thresholds` such that it and every smaller candidate are acceptable, or None (run the backbone alone).
    gaps, sems_k: [len(thresholds), n] (threshold_statistics per candidate); a candidate is acceptable where gap_k + sems * sem_k <=
    tolerance at EVERY grid timestep -- one global threshold serves all steps.  Pure numpy."""
    th = np.asarray(thresholds, np.float64)
    g, e = np.asarray(gaps, np.float64), np.asarray(sems_k, np.float64)
    if th.ndim != 1 or g.shape != e.shape or g.ndim != 2 or len(g) != len(th):
        raise ValueError("one row of gaps and sems per threshold")
    ok = (g + float(sems) * e <= float(tolerance)).all(axis=1)
    best = None
    for j in np.argsort(th, kind="stable"):
        if not ok[j]:
            break
        best = float(th[j])
    return best


def calibration(pred, target):
    """Per layer, over images x timesteps: how well probe l's prediction pred [n, depth, N] matches its training target target[:, :depth]
    ([n, depth + 1, N] or [n, depth, N]).  Returns a dict of lists: mean_predicted, mean_target, rmse, pearson_r (nan where a side is constant)."""
    p, t = np.asarray(pred, np.float64), np.asarray(target, np.float64)[:, :np.shape(pred)[1]]
    if p.ndim != 3 or p.shape != t.shape:
        raise ValueError("pred [timesteps, depth, images] and target [timesteps, depth (+ 1), images]")
    p, t = p.transpose(1, 0, 2).reshape(p.shape[1], -1), t.transpose(1, 0, 2).reshape(p.shape[1], -1)
    dp, dt = p - p.mean(axis=1, keepdims=True), t - t.mean(axis=1, keepdims=True)
    den = np.sqrt((dp * dp).sum(axis=1) * (dt * dt).sum(axis=1))
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(den > 0, (dp * dt).sum(axis=1) / den, np.nan)
    return {"mean_predicted": p.mean(axis=1).tolist(), "mean_target": t.mean(axis=1).tolist(),
            "rmse": np.sqrt(((p - t) ** 2).mean(axis=1)).tolist(), "pearson_r": r.tolist()}


def candidate_thresholds(pred, thresholds=None, num_thresholds=None):
    """--thresholds as given (finite, >= 0: below 0 the reference's argmax quirk exits at layer 0), or --num_thresholds N: the distinct
    N quantiles of the recorded predictions as float32, floored at 0.  Sorted ascending."""
    if (thresholds is None) == (num_thresholds is None):
        raise ValueError("give --thresholds or --num_thresholds, one of them")
    if thresholds is not None:
        th = [float(v) for v in thresholds]
        if not th or any(not math.isfinite(v) or v < 0 for v in th):
            raise ValueError("--thresholds must be finite and not negative (below 0 the sampler's rule exits at layer 0)")
        return sorted(set(float(F32(v)) for v in th))
    if num_thresholds < 1:
        raise ValueError(f"--num_thresholds {num_thresholds} must be at least 1")
    q = np.quantile(np.asarray(pred, np.float64).ravel(), np.linspace(0.0, 1.0, int(num_thresholds)))
    return sorted(set(float(v) for v in np.maximum(q, 0.0).astype(F32)))


def get_args(argv=None):
    p = ArgumentParser(description=__doc__.split("\n\n")[0])
    def own(p, after):
        if after == "checkpoint_path":
            p.add_argument("--parametrization", type=str, required=True, help=f"one of {PARAMETRIZATIONS}")
        if after == "stride":
            p.add_argument("--thresholds", type=float, nargs="+", default=None, metavar="T", help="the candidate thresholds")
            p.add_argument("--num_thresholds", type=int, default=None, metavar="N",
                           help="candidates = the distinct N quantiles of the recorded predictions (default 32 where --thresholds is not given)")
    add_scan_options(p, "Path to yaml config file (with model_params.classifier_type)", "Path to checkpoint of the early-exit model",
                     "largest acceptable relative gap of the realised error over the backbone's", own)
    return p.parse_args(argv)


def validate(args, config):
    """Every option check that needs no image and no GPU: ValueError on a bad combination.  Returns the grid.  --num_thresholds takes its
    default of 32 here."""
    from .config import ModelParams
    if args.parametrization not in PARAMETRIZATIONS:
        raise ValueError(f"--parametrization must be one of {PARAMETRIZATIONS} (the early-exit trainer allows no other), not {args.parametrization!r}")
    grid = scan_timesteps(args.timesteps, args.stride)
    if args.thresholds is not None and args.num_thresholds is not None:
        raise ValueError("--thresholds and --num_thresholds are exclusive")
    if args.thresholds is None and args.num_thresholds is None:
        args.num_thresholds = 32
    candidate_thresholds(np.zeros(1), args.thresholds, args.num_thresholds)        # (the list's own checks)
    check_numbers(args)
    check_label_options(args)
    params = dict(config["model_params"])
    if "classifier_type" not in params:
        raise ValueError("--config_path has no model_params.classifier_type: not an early-exit model (switch_scan scans plain models)")
    params.pop("classifier_type")
    mp = ModelParams.from_dict({**config, "model_params": params})
    if "autoencoder" in config:
        raise ValueError("latent early-exit models are not supported by this tool")
    check_labels(args, mp.num_classes)
    check_images_path(args.images, mp.in_chans)
    return grid


def scan(model, x0, y, rows, seed, repeats, batch_size, use_graph=True):
    """(mse [repeats, n, depth + 1, N], target (the same), predicted [repeats, n, depth, N]) float32 of the engine Model on x0
    [N, C, S, S] (numpy), in batches of batch_size; image i under seed + i whatever its batch; repeat r draws with Philox counters r n + k."""
    from .engine import scan_exits_loop
    n, N, depth = len(rows["t"]), len(x0), model.mp.depth
    mse, target = (np.zeros((repeats, n, depth + 1, N), F32) for _ in range(2))
    pred = np.zeros((repeats, n, depth, N), F32)
    for xb, yb, at in batches(model.ctx, x0, y, seed, batch_size):
        for r in range(repeats):
            out = scan_exits_loop(model.ctx, model, xb, rows, y=yb, counter_base=r * n, use_graph=use_graph)
            for dst, src in zip((mse, target, pred), out):
                dst[r, :, :, at] = src.cpu().numpy()
    return mse, target, pred


def summarize(args, grid, mse, target, pred):
    """exits.json from the saved arrays: per-timestep per-exit means, calibration, the per-candidate table, the suggestion.  The exit rule
    is replayed per repeat (the sampler decides on one draw); the realised and the backbone's error are then averaged per image."""
    R, n, E, N = mse.shape
    depth = E - 1
    thresholds = candidate_thresholds(pred, args.thresholds, args.num_thresholds)
    m64 = mse.astype(np.float64)
    table, gaps, sems_k = [], [], []
    for thr in thresholds:
        idx = np.stack([simulate_exits(pred[r], thr) for r in range(R)])                          # [R, n, N]
        gap, sem, blocks = threshold_statistics(m64, idx)
        ok = bool((gap + args.sems * sem <= args.tolerance).all())
        gaps.append(gap); sems_k.append(sem)
        table.append({"threshold": thr, "gap": gap.tolist(), "sem": sem.tolist(), "max_gap": float(gap.max()), "acceptable": ok,
                      "blocks_fraction": blocks, "mean_exit_by_timestep": idx.mean(axis=(0, 2)).tolist()})
    best = suggest_threshold(thresholds, gaps, sems_k, args.tolerance, args.sems)
    blocks = next((row["blocks_fraction"] for row in table if row["threshold"] == best), 1.0)
    return {"parametrization": args.parametrization, "timesteps": [int(t) for t in grid], "images": int(N), "repeats": int(R), "seed": int(args.seed),
            "precision": args.precision, "depth": int(depth), "tolerance": float(args.tolerance), "sems": float(args.sems),
            "mean_mse": m64.mean(axis=(0, 3)).tolist(), "mean_target": target.astype(np.float64).mean(axis=(0, 3)).tolist(),
            "mean_predicted": pred.astype(np.float64).mean(axis=(0, 3)).tolist(),
            "calibration": calibration(pred.reshape(R * n, depth, N), target.reshape(R * n, E, N)),
            "candidates": table, "threshold": best,
            "advice": (f"--threshold {best:.9g} (about {100.0 * blocks:.1f} % of the blocks)" if best is not None
                       else "run the backbone alone (no candidate threshold keeps the realised error within the tolerance at every timestep)")}


def main(argv=None):
    from .config import ModelParams, load_config
    from .early_exit import EarlyExitUViT
    from .sampler import load_checkpoint
    from .step_plan import scan_rows
    from .uvit import UViT
    args = get_args(argv)
    config = load_config(args.config_path)
    grid = validate(args, config)
    params = dict(config["model_params"])
    classifier_type = params.pop("classifier_type")
    mp = ModelParams.from_dict(config)
    x0 = load_images(args.images, mp.in_chans, mp.img_size)
    y = load_labels(args, len(x0), mp.num_classes)
    out = Path(args.output_folder)
    out.mkdir(parents=True, exist_ok=True)
    bs = min(args.batch_size, len(x0))
    model = EarlyExitUViT(UViT(**params, precision=args.precision, max_batch=bs), classifier_type)
    model.load_state_dict(load_checkpoint(args.checkpoint_path))
    model = model.eval().to("cuda")
    rows = scan_rows(grid, args.parametrization)
    mse, target, pred = scan(model.engine_model(bs), x0, y, rows, args.seed, args.repeats, bs, use_graph=not args.no_graph)
    np.savez(out / "exits.npz", timesteps=np.asarray(grid, np.int64), image_seeds=np.arange(len(x0), dtype=np.int64) + int(args.seed),
             mse=mse, target=target, predicted=pred)
    summary = summarize(args, grid, mse, target, pred)
    (out / "exits.json").write_text(json.dumps(summary, indent=1) + "\n")
    for k, t in enumerate(grid):
        print(f"t = {t:3d}  mse by exit  " + " ".join(f"{v:.5f}" for v in summary["mean_mse"][k]))
    cal = summary["calibration"]
    for l in range(summary["depth"]):
        print(f"probe {l:2d}  predicted {cal['mean_predicted'][l]:.5f}  target {cal['mean_target'][l]:.5f}  rmse {cal['rmse'][l]:.5f}  r {cal['pearson_r'][l]:+.3f}")
    for row in summary["candidates"]:
        print(f"threshold {row['threshold']:.6g}  max gap {row['max_gap']:+.4f}  blocks {row['blocks_fraction']:.3f}{'' if row['acceptable'] else '  *'}")
    print(summary["advice"])


if __name__ == "__main__":
    main()
