"""Resampling jumps in the device loop: what a jump row costs beside a step row, and the one device loop against the loop cut at every jump.

    python tools/resample_bench.py [--ddim_steps 50] [--jump 10] [--count 10] [--warmup 1] [--repeats 3]
    python tools/resample_bench.py --summarize-trace DIR     (DIR: a rocprofv3 --kernel-trace --stats run of this tool)

bench.py's CelebA pair (uvit_celeba_3 -> uvit_celeba, synthetic weights, bf16, hipGraph replay, B = 128, the late model below
t = 1000 - 300), DDIM with a half-image mask.  Four runs alternate, `repeats` times each, each timed by hipEvents on its stream:
  base   the jump-free DDIM loop with the region (dd_sample_affine_region): ms per step row
  walk   RePaint's (j, r) walk as ONE device loop (dd_sample_affine_walk): S step rows and J jump rows
  cut    the same walk cut behind every jump, one dd_sample_affine_walk call per descent (what a caller had to do before the walk
         was in the driver: every call re-stages x and the region, re-derives the graphs' keys and forks and joins the chains)
  jumps  the walk's J jump rows alone, as one call: ms per jump row (two launches per chain and row, no model)
walk and cut compute the same images bit for bit (checked).  ms per step row of the walk = (walk - jumps) / S; it differs from base's,
whose steps are another mix of the two models (every jump of this walk lies below the switch, so the repeated steps are the late model's).
Writes profiles/resample/resample_bench.json.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

from loop_bench_support import LoopTimer, spread, synthetic_pair  # noqa: E402

OUT = REPO / "profiles" / "resample"
FIRST, LATE, B, SEEDS, T_SWITCH = "uvit_celeba_3.yaml", "uvit_celeba.yaml", 128, (1235, 1234), 300


def bench(a):
    import numpy as np
    import torch
    from duodiff_amd import _lib, step_plan as sp
    from duodiff_amd.engine import KnownRegion, sample_affine_region_loop, sample_affine_walk_loop
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench.py needs an MI355X: the engine has no CPU path")
    torch.cuda.set_device(0)
    dev = "cuda:0"
    es, ef, _, mp = synthetic_pair(FIRST, LATE, SEEDS, B)
    ctx = es.ctx
    kw = dict(parametrization="predict_noise", has_late=True, t_switch=T_SWITCH, use_ddim=True, ddim_steps=a.ddim_steps)
    base, walk = sp.step_plan(**kw), sp.step_plan(**kw, resample_jump=a.jump, resample_count=a.count)
    n_base, jump = len(base.rows["t"]), walk.rows["jump"]
    S, J = int((jump == 0).sum()), int(jump.sum())
    cuts = [0, *(int(k) + 1 for k in np.nonzero(jump)[0]), len(jump)]
    g = torch.Generator().manual_seed(0)
    x_T = torch.randn(B, mp.in_chans, mp.img_size, mp.img_size, generator=g).to(dev)
    x0 = torch.randn(B, mp.in_chans, mp.img_size, mp.img_size, generator=g).to(dev)
    mask = torch.zeros(B, 1, mp.img_size, mp.img_size, device=dev)
    mask[..., : mp.img_size // 2] = 1
    regions = {name: KnownRegion(x0, mask, *sp.known_rows(p)) for name, p in (("base", base), ("walk", walk))}
    x = x_T.clone()
    timer = LoopTimer(ctx)
    r, w = base.rows, walk.rows

    def loop(mode):
        def run(stream):
            if mode == "base":
                sample_affine_region_loop(ctx, es, ef, x, regions["base"], r["t"], r["a"], r["b"], r["c"], r["noise"],
                                          switch_after=base.switch_after, seed=0, stream=stream)
                return
            if mode == "jumps":
                sample_affine_walk_loop(ctx, es, ef, x, only_jumps, seed=0, stream=stream)
                return
            for k0, k1 in ((0, len(jump)),) if mode == "walk" else zip(cuts[:-1], cuts[1:]):
                if k1 > k0:
                    reg = regions["walk"]._replace(ka=regions["walk"].ka[k0:k1], kb=regions["walk"].kb[k0:k1])
                    sample_affine_walk_loop(ctx, es, ef, x, {k: v[k0:k1] for k, v in w.items()}, region=reg, seed=0, counter_base=k0, stream=stream)
        return run

    only_jumps = {k: v[jump == 1] for k, v in w.items()}
    modes = ("base", "walk", "cut", "jumps")
    images = {}
    for _ in range(a.warmup):
        for mode in modes:
            timer.run(loop(mode), x, x_T, mode, timed=False)
            images[mode] = x.clone()
    assert torch.equal(images["walk"], images["cut"]), "the cut walk differs from the one device loop"
    res, chains = {m: [] for m in modes}, {}
    for rep in range(a.repeats):
        for mode in modes:
            ms, chains[mode] = timer.run(loop(mode), x, x_T, mode)
            res[mode].append(ms)
            print(f"repeat {rep} {mode}: {ms:.2f} ms, chains {chains[mode]}", flush=True)
    med = {m: statistics.median(v) for m, v in res.items()}
    step_ms = med["base"] / n_base
    out = {"_build_id": _lib.load().dd_build_id().decode(),
           "config": {"precision": "bf16", "hipgraph": True, "weights": "synthetic", "pair": f"{FIRST} -> {LATE} below t = {1000 - T_SWITCH}",
                      "B_images": B, "ddim_steps": a.ddim_steps, "grid_steps": n_base, "jump": a.jump, "count": a.count, "step_rows": S,
                      "jump_rows": J, "calls_of_the_cut_walk": len(cuts) - 1, "mask": "left half known", "warmup_runs": a.warmup,
                      "repeats": a.repeats, "order": "alternating base / walk / cut / jumps", "timing": "hipEvents around each run on its stream",
                      "date": time.strftime("%Y-%m-%d")},
           "base": {"chains": chains["base"], "ms": spread(res["base"]), "ms_per_step_row": step_ms},
           "walk": {"chains": chains["walk"], "ms": spread(res["walk"]), "ms_per_row": med["walk"] / (S + J),
                    "ms_per_step_row": (med["walk"] - med["jumps"]) / S, "images_per_s": B / (med["walk"] / 1e3)},
           "jumps": {"chains": chains["jumps"], "ms": spread(res["jumps"]), "ms_per_jump_row": med["jumps"] / J if J else None},
           "cut": {"chains": chains["cut"], "ms": spread(res["cut"]), "images_per_s": B / (med["cut"] / 1e3),
                   "extra_ms_per_call_over_walk": (med["cut"] - med["walk"]) / max(len(cuts) - 2, 1)}}
    print(json.dumps(out, indent=1))
    if not a.no_json:
        OUT.mkdir(parents=True, exist_ok=True)
        (OUT / "resample_bench.json").write_text(json.dumps(out, indent=1) + "\n")


def summarize_trace(d):
    """Duration per launch of jump_kernel and jump_advance_kernel by grid size (a half-batch chain's grid and the whole batch's apart)"""
    from duodiff_amd import _lib
    trace = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not trace:
        raise SystemExit(f"no kernel_trace.csv under {d}")
    durs = {}
    for f in trace:
        for r in csv.DictReader(open(f)):
            for name in ("jump_kernel", "jump_advance_kernel"):
                if name + "<" in r["Kernel_Name"] or name + "(" in r["Kernel_Name"] or r["Kernel_Name"].endswith(name):
                    grid = int(r["Grid_Size_X"]) if "Grid_Size_X" in r else -1
                    durs.setdefault(name, {}).setdefault(grid, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = {"_build_id": _lib.load().dd_build_id().decode(),
           "source": "rocprofv3 --kernel-trace --stats of tools/resample_bench.py (its own run); microseconds per launch by grid size (work-items)"}
    for name, by_grid in durs.items():
        out[name] = {str(k): {"launches": len(v), "mean_us": statistics.mean(v), "median_us": statistics.median(v), "min_us": min(v)}
                     for k, v in sorted(by_grid.items())}
    print(json.dumps(out, indent=1))
    OUT.mkdir(parents=True, exist_ok=True)
    (OUT / "jump_kernel_trace.json").write_text(json.dumps(out, indent=1) + "\n")


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--ddim_steps", type=int, default=50)
    p.add_argument("--jump", type=int, default=10)
    p.add_argument("--count", type=int, default=10)
    p.add_argument("--warmup", type=int, default=1, help="untimed runs of each loop first (graph captures, code-object loads)")
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--no_json", action="store_true", help="print only (the profiled run)")
    p.add_argument("--summarize-trace", dest="trace", default=None)
    a = p.parse_args(argv)
    if a.trace:
        summarize_trace(a.trace)
    else:
        bench(a)


if __name__ == "__main__":
    main()
