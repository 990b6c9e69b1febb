"""Block caching against the uncached loop: images per second, and what a refresh step and a reuse step cost.

    python tools/cache_bench.py [--warmup 2] [--repeats 5]

The CelebA full model (configs/uvit_celeba.yaml, depth 13; synthetic weights, bf16, hipGraph replay, device Philox), B = 128, on two
loops: DDIM with 50 evaluations (ddim_steps = 51) and the first 100 DDPM steps.  Both run through step_plan's rows: the uncached plan on
dd_sample_affine, then (K, N) in {(1, 2), (2, 3), (3, 5)} with order 0 and order 1 on dd_sample_affine_cached.  All settings of a loop
alternate in one process, `repeats` times each, each run timed by hipEvents on its stream.  Every setting runs on an engine model of its
own (the same weights): a model keeps one captured step per loop kind, and alternating settings on one model would re-capture inside the
timed calls.
ms per step: the cached loop of R refresh and U reuse steps takes T = R r + U u.  r is measured by the same loop with N = 1 (every step
a refresh: the full forward with the seam's skip_linear unfused and the store of y_deep), u = (T - R r) / U.  dd_last_sample_timing
splits a loop by model, not by row kind, so it does not give this split.
Image quality under caching is not measured here (synthetic weights).  Writes profiles/cache/cache_bench.json.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

from loop_bench_support import DEV, LoopTimer, spread  # noqa: E402

OUT = REPO / "profiles" / "cache"
CONFIG, B, SEED = "uvit_celeba.yaml", 128, 1234
SETTINGS = [(1, 2), (2, 3), (3, 5)]
LOOPS = {"ddim50": dict(use_ddim=True, ddim_steps=51), "ddpm100": dict(num_steps=100)}


def bench(a):
    import torch
    from duodiff_amd import _lib
    from duodiff_amd import step_plan as sp
    from duodiff_amd.config import ModelParams, load_config
    from duodiff_amd.engine import sample_affine_cached_loop, sample_affine_loop
    from duodiff_amd.uvit import UViT
    from duodiff_amd.weights import synthetic_state_dict
    if not torch.cuda.is_available():
        raise SystemExit("cache_bench.py needs an MI355X: the engine has no CPU path")
    torch.cuda.set_device(0)
    mp = ModelParams.from_dict(load_config(REPO / "configs" / CONFIG))
    sd = synthetic_state_dict(mp, SEED)

    def engine_model():
        return UViT(**mp.as_dict(), precision="bf16", max_batch=B).load_state_dict(sd).to(DEV).engine_model(B)

    ems = {}
    x_T = torch.randn(B, mp.in_chans, mp.img_size, mp.img_size, generator=torch.Generator().manual_seed(0)).to(DEV)
    x = x_T.clone()
    timer = None
    out = {"_build_id": _lib.load().dd_build_id().decode(),
           "config": {"model": CONFIG, "depth": mp.depth, "B": B, "precision": "bf16", "hipgraph": True, "noise": "device Philox",
                      "weights": "synthetic", "warmup_runs": a.warmup, "repeats": a.repeats, "order": "all settings of a loop alternate",
                      "timing": "hipEvents around each loop call on its stream", "date": time.strftime("%Y-%m-%d"),
                      "split": "ms_refresh from the N = 1 run of the same K; ms_reuse = (T - R ms_refresh) / U",
                      "image_quality": "not measured (synthetic weights)"}}
    for loop_name, plan_kw in LOOPS.items():
        # name -> (K, order, plan); K None: the uncached affine loop on the same rows
        runs = {"uncached": (None, 0, sp.step_plan("predict_noise", **plan_kw, cache_blocks=1, cache_interval=1))}
        for K, N in SETTINGS:
            runs[f"K{K}_refresh_only"] = (K, 0, sp.step_plan("predict_noise", **plan_kw, cache_blocks=K, cache_interval=1))
            for order in (0, 1):
                runs[f"K{K}_N{N}_order{order}"] = (K, order, sp.step_plan("predict_noise", **plan_kw, cache_blocks=K, cache_interval=N, cache_order=order))

        for name in runs:
            if name not in ems:
                ems[name] = engine_model()
        ctx = ems["uncached"].ctx
        timer = timer or LoopTimer(ctx)

        def run(name, timed):
            K, order, plan = runs[name]
            r, em = plan.rows, ems[name]

            def loop(stream):
                if K is None:
                    sample_affine_loop(ctx, em, None, x, r["t"], r["a"], r["b"], r["c"], r["noise"], seed=0, noise="philox", stream=stream)
                else:
                    sample_affine_cached_loop(ctx, em, None, x, r, blocks=K, order=order, seed=0, noise="philox", stream=stream)
            return timer.run(loop, x, x_T, (loop_name, name), timed=timed)

        for _ in range(a.warmup):
            for name in runs:
                run(name, False)
        ms = {name: [] for name in runs}
        chains = {}
        for rep in range(a.repeats):
            for name in runs:
                t, chains[name] = run(name, True)
                ms[name].append(t)
                print(f"{loop_name} repeat {rep} {name}: {t:.2f} ms, {B / (t / 1e3):.2f} images/s, chains {chains[name]}", flush=True)
        res = {}
        base = float(np.median(ms["uncached"]))
        for name, (K, order, plan) in runs.items():
            n = len(plan.rows["t"])
            med = float(np.median(ms[name]))
            rec = {"steps": n, "chains": chains[name], "ms_total": spread(ms[name]), "images_per_s": spread([B / (t / 1e3) for t in ms[name]]),
                   "ms_per_step": med / n, "speedup_over_uncached": base / med}
            if K is not None and "refresh_only" not in name:
                R = int((plan.rows["cache"] == 0).sum())
                U = n - R
                r_ms = float(np.median(ms[f"K{K}_refresh_only"])) / n
                rec.update(refresh_steps=R, reuse_steps=U, ms_refresh=r_ms, ms_reuse=(med - R * r_ms) / U)
            res[name] = rec
        out[loop_name] = res
    print(json.dumps(out, indent=1))
    if not a.no_json:
        OUT.mkdir(parents=True, exist_ok=True)
        (OUT / "cache_bench.json").write_text(json.dumps(out, indent=1) + "\n")


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--warmup", type=int, default=2, help="untimed runs of each setting first (graph captures, code-object loads)")
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--no_json", action="store_true", help="print only")
    bench(p.parse_args(argv))


if __name__ == "__main__":
    main()
