"""DPM-Solver++ multistep sampling against DDIM with the same number of model evaluations: what the history register costs per step.

    python tools/multistep_bench.py [--evals 20] [--warmup 3] [--repeats 3]
    python tools/multistep_bench.py --summarize-trace DIR     (DIR: a rocprofv3 --kernel-trace --stats run of this tool)

Two of bench.py's pairs (synthetic weights, bf16, hipGraph replay, device Philox, the late model from 30 % of the steps on):
  celeba       uvit_celeba_3 -> uvit_celeba,             B = 128, unguided
  imagenet256  uvit_imagenet256_3 -> uvit_imagenet256,   B = 32, guided at scale 0.4 (null label 1000, 64 backbone rows)
On each, a 20-evaluation DPM-Solver++(2M) run (dd_sample_multistep, grid sampler.multistep_grid) and a DDIM run with the same 20
evaluations (ddim_steps = 21, dd_sample_affine) alternate, `repeats` times each, each run timed by hipEvents on its stream.  The
backbone work is identical; the step's last kernel differs (final_*_kernel<..., true> also reads and writes h).
Writes profiles/multistep/multistep_bench.json.
"""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

from loop_bench_support import LoopTimer, spread, synthetic_pair  # noqa: E402

OUT = REPO / "profiles" / "multistep"
SCALE, NULL = 0.4, 1000
PAIRS = {
    "celeba": dict(first="uvit_celeba_3.yaml", late="uvit_celeba.yaml", B=128, guidance=None, seeds=(1235, 1234)),
    "imagenet256": dict(first="uvit_imagenet256_3.yaml", late="uvit_imagenet256.yaml", B=32, guidance=(SCALE, NULL), seeds=(1237, 1236)),
}


def bench_pair(name, spec, a):
    import torch
    from duodiff_amd import sampler
    from duodiff_amd.engine import sample_affine_loop, sample_multistep_loop

    dev = "cuda:0"
    B, guidance = spec["B"], spec["guidance"]
    rows = 2 * B if guidance else B
    es, ef, _, mp_f = synthetic_pair(spec["first"], spec["late"], spec["seeds"], rows)
    ctx = es.ctx
    N = a.evals
    k_sw = max(1, round(0.3 * N))
    ms_rows = sampler.multistep_coefficients("dpmsolver++", sampler.multistep_grid(N), 2)
    ts = np.linspace(0, 999, N + 1).astype(int)[::-1]                        # DDIM, ddim_steps = N + 1: N evaluations
    co = [sampler.affine_coefficients("ddim", int(t), int(s), 0.0) for t, s in zip(ts[:-1], ts[1:])]
    g = torch.Generator().manual_seed(0)
    S, Cc = mp_f.img_size, mp_f.in_chans
    x_T = torch.randn(B, Cc, S, S, generator=g).to(dev)
    y = torch.randint(0, 1000, (B,), generator=g).to(dev) if mp_f.num_classes > 0 else None
    x, h = x_T.clone(), torch.zeros_like(x_T)
    timer = LoopTimer(ctx)

    def run(kind, timed):
        def loop(stream):
            if kind == "dpmsolver++":
                sample_multistep_loop(ctx, es, ef, x, h, ms_rows, switch_after=k_sw, y=y, seed=0, noise="philox", stream=stream,
                                      guidance=guidance)
            else:
                sample_affine_loop(ctx, es, ef, x, [float(t) for t in ts[:-1]], [c[0] for c in co], [c[1] for c in co], [c[2] for c in co],
                                   [0] * N, switch_after=k_sw, y=y, seed=0, noise="philox", stream=stream, guidance=guidance)
        return timer.run(loop, x, x_T, (name, kind), h=h, timed=timed)

    kinds = ("dpmsolver++", "ddim")
    for _ in range(a.warmup):
        for kind in kinds:
            run(kind, False)
    res = {k: {"ms_per_step": [], "images_per_s": []} for k in kinds}
    chains = {}
    for r in range(a.repeats):
        for kind in kinds:
            ms, chains[kind] = run(kind, True)
            res[kind]["ms_per_step"].append(ms / N)
            res[kind]["images_per_s"].append(B / (ms / 1e3))                # one N-evaluation sample of B images
            print(f"{name} repeat {r} {kind}: {ms / N:.4f} ms/step, {B / (ms / 1e3):.2f} images/s, chains {chains[kind]}", flush=True)
    out = {"pair": f"{spec['first']} (first {k_sw} steps) -> {spec['late']}", "B_images": B, "backbone_rows": rows,
           "guidance": {"scale": guidance[0], "null_label": guidance[1]} if guidance else None, "evaluations": N}
    for kind in kinds:
        out[kind] = {"chains": chains[kind], "ms_per_step": spread(res[kind]["ms_per_step"]), "images_per_s": spread(res[kind]["images_per_s"])}
    out["dpm_over_ddim_ms_per_step"] = out["dpmsolver++"]["ms_per_step"]["median"] / out["ddim"]["ms_per_step"]["median"]
    out["target_met"] = out["dpm_over_ddim_ms_per_step"] <= 1.01
    del es, ef
    torch.cuda.empty_cache()
    return out


def bench(a):
    import torch
    from duodiff_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("multistep_bench.py needs an MI355X: the engine has no CPU path")
    torch.cuda.set_device(0)
    out = {"_build_id": _lib.load().dd_build_id().decode(),
           "config": {"precision": "bf16", "hipgraph": True, "noise": "device Philox (the ODE / eta = 0 rows draw none)",
                      "weights": "synthetic", "warmup_runs": a.warmup, "repeats": a.repeats, "order": "alternating DPM-Solver++ / DDIM",
                      "timing": "hipEvents around each loop call on its stream", "date": time.strftime("%Y-%m-%d"),
                      "target": "DPM-Solver++ ms/step <= 1.01 x DDIM ms/step at the same evaluations"}}
    for name in a.pairs:
        out[name] = bench_pair(name, PAIRS[name], a)
    print(json.dumps(out, indent=1))
    if not a.no_json:
        OUT.mkdir(parents=True, exist_ok=True)
        (OUT / "multistep_bench.json").write_text(json.dumps(out, indent=1) + "\n")


_TARGS = re.compile(r"final_(tiled_)?kernel<([^>]*)>|final_(tiled_)?kernelI(\w+?)EEv")


def summarize_trace(d):
    """Median duration per launch of each final kernel instantiation, and multistep (H = true) over affine (H = false) per shape."""
    from duodiff_amd import _lib
    trace = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not trace:
        raise SystemExit(f"no kernel_trace.csv under {d}")
    durs = {}
    for f in trace:
        for r in csv.DictReader(open(f)):
            n = r["Kernel_Name"]
            if "final_tiled_kernel" in n:
                durs.setdefault(n, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = {"_build_id": _lib.load().dd_build_id().decode(),
           "source": "rocprofv3 --kernel-trace --stats of tools/multistep_bench.py (its own run); durations in microseconds",
           "kernels": {}, "multistep_over_affine_median": {}}
    for n, v in sorted(durs.items()):
        out["kernels"][n] = {"launches": len(v), "mean_us": statistics.mean(v), "median_us": statistics.median(v), "min_us": min(v)}

    def split(n):       # (shape key, H) from "...<3, 4, false, true>" or the mangled "...ILi3ELi4ELb0ELb1EEv..."
        m = _TARGS.search(n)
        if not m:
            return None
        if m.group(2) is not None:
            args = [s.strip() for s in m.group(2).split(",")]
            return ("tiled " if m.group(1) else "") + ", ".join(args[:-1]), args[-1] in ("true", "1")
        args = m.group(4)
        return ("tiled " if m.group(3) else "") + args[:-4], args.endswith("Lb1")
    by = {}
    for n, st in out["kernels"].items():
        s = split(n)
        if s:
            by.setdefault(s[0], {})[s[1]] = st["median_us"]
    for shape, v in by.items():
        if True in v and False in v:
            out["multistep_over_affine_median"][shape] = v[True] / v[False]
    out["target"] = "multistep final kernel <= 1.25 x the affine one"
    out["target_met"] = bool(out["multistep_over_affine_median"]) and all(r <= 1.25 for r in out["multistep_over_affine_median"].values())
    print(json.dumps(out, indent=1))
    OUT.mkdir(parents=True, exist_ok=True)
    (OUT / "final_kernel_trace.json").write_text(json.dumps(out, indent=1) + "\n")


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--evals", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3, help="untimed runs of each loop first (graph captures, code-object loads)")
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--pairs", nargs="+", default=list(PAIRS), choices=list(PAIRS))
    p.add_argument("--no_json", action="store_true", help="print only (the profiled run)")
    p.add_argument("--summarize-trace", dest="trace", default=None)
    a = p.parse_args(argv)
    if a.trace:
        summarize_trace(a.trace)
    else:
        bench(a)


if __name__ == "__main__":
    main()
