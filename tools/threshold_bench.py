"""x0 thresholding of the multistep loop against the plain loop: what the second launch of a thresholded step costs.

    python tools/threshold_bench.py [--evals 20] [--warmup 3] [--repeats 5]
    python tools/threshold_bench.py --summarize-trace DIR     (DIR: a rocprofv3 --kernel-trace --stats run of this tool)

bench.py's CelebA pair (uvit_celeba_3 -> uvit_celeba, synthetic weights, bf16, hipGraph replay, B = 128, the late model from 30 % of the
steps on), a 20-evaluation DPM-Solver++(2M) run: the plain loop (dd_sample_multistep, folded rows), the static clip to [-1, 1] and
dynamic thresholding at quantile 0.995 (dd_sample_multistep_threshold, unfolded rows) alternate, `repeats` times each, each run timed by
hipEvents on its stream.  The backbone work is identical; a thresholded step's output head writes the model output to a scratch image
and threshold_step_kernel, one workgroup per image, finishes the step.
Writes profiles/threshold/threshold_bench.json.
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

OUT = REPO / "profiles" / "threshold"
FIRST, LATE, B, SEEDS = "uvit_celeba_3.yaml", "uvit_celeba.yaml", 128, (1235, 1234)


def bench(a):
    import torch
    from duodiff_amd import _lib, sampler
    from duodiff_amd.engine import X0Threshold, sample_multistep_loop, sample_multistep_threshold_loop
    if not torch.cuda.is_available():
        raise SystemExit("threshold_bench.py needs an MI355X: the engine has no CPU path")
    torch.cuda.set_device(0)
    dev = "cuda:0"
    es, ef, _, mp_f = synthetic_pair(FIRST, LATE, SEEDS, B)
    ctx = es.ctx
    N = a.evals
    k_sw = max(1, round(0.3 * N))
    grid = sampler.multistep_grid(N)
    folded = sampler.multistep_coefficients("dpmsolver++", grid, 2)
    unfolded = sampler.multistep_coefficients("dpmsolver++", grid, 2, unfolded=True)
    modes = {"plain": None, "static": X0Threshold("static", range=1.0), "dynamic": X0Threshold("dynamic", quantile=0.995)}
    x_T = torch.randn(B, mp_f.in_chans, mp_f.img_size, mp_f.img_size, generator=torch.Generator().manual_seed(0)).to(dev)
    x, h = x_T.clone(), torch.zeros_like(x_T)
    timer = LoopTimer(ctx)

    def run(mode, timed):
        def loop(stream):
            kw = dict(switch_after=k_sw, seed=0, noise="philox", stream=stream)
            if modes[mode] is None:
                sample_multistep_loop(ctx, es, ef, x, h, folded, **kw)
            else:
                sample_multistep_threshold_loop(ctx, es, ef, x, h, unfolded, modes[mode], **kw)
        return timer.run(loop, x, x_T, mode, h=h, timed=timed)

    for _ in range(a.warmup):
        for mode in modes:
            run(mode, False)
    res, chains = {m: [] for m in modes}, {}
    for r in range(a.repeats):
        for mode in modes:
            ms, chains[mode] = run(mode, True)
            res[mode].append(ms / N)
            print(f"repeat {r} {mode}: {ms / N:.4f} ms/step, chains {chains[mode]}", flush=True)
    out = {"_build_id": _lib.load().dd_build_id().decode(),
           "config": {"precision": "bf16", "hipgraph": True, "weights": "synthetic", "pair": f"{FIRST} (first {k_sw} steps) -> {LATE}",
                      "B_images": B, "evaluations": N, "warmup_runs": a.warmup, "repeats": a.repeats, "order": "alternating plain / static / dynamic",
                      "timing": "hipEvents around each loop call on its stream", "date": time.strftime("%Y-%m-%d")}}
    for mode in modes:
        out[mode] = {"chains": chains[mode], "ms_per_step": spread(res[mode])}
    for mode in ("static", "dynamic"):
        out[mode]["extra_ms_per_step_over_plain"] = out[mode]["ms_per_step"]["median"] - out["plain"]["ms_per_step"]["median"]
    print(json.dumps(out, indent=1))
    if not a.no_json:
        OUT.mkdir(parents=True, exist_ok=True)
        (OUT / "threshold_bench.json").write_text(json.dumps(out, indent=1) + "\n")


def summarize_trace(d):
    """Duration per launch of threshold_step_kernel by grid size (a half-batch chain's grid and the whole batch's apart)"""
    from duodiff_amd import _lib
    trace = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not trace:
        raise SystemExit(f"no kernel_trace.csv under {d}")
    durs = {}
    for f in trace:
        for r in csv.DictReader(open(f)):
            if "threshold_step_kernel" in r["Kernel_Name"]:
                images = int(r["Grid_Size_X"]) // max(int(r["Workgroup_Size_X"]), 1) if "Grid_Size_X" in r else -1
                durs.setdefault(images, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = {"_build_id": _lib.load().dd_build_id().decode(),
           "source": "rocprofv3 --kernel-trace --stats of tools/threshold_bench.py (its own run); microseconds per launch by images per grid",
           "threshold_step_kernel": {str(k): {"launches": len(v), "mean_us": statistics.mean(v), "median_us": statistics.median(v), "min_us": min(v)}
                                     for k, v in sorted(durs.items())}}
    print(json.dumps(out, indent=1))
    OUT.mkdir(parents=True, exist_ok=True)
    (OUT / "threshold_kernel_trace.json").write_text(json.dumps(out, indent=1) + "\n")


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--evals", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3, help="untimed runs of each loop first (graph captures, code-object loads)")
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--no_json", action="store_true", help="print only (the profiled run)")
    p.add_argument("--summarize-trace", dest="trace", default=None)
    a = p.parse_args(argv)
    if a.trace:
        summarize_trace(a.trace)
    else:
        bench(a)


if __name__ == "__main__":
    main()
