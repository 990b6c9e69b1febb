"""Classifier-free guidance on the ImageNet-256 latent pair: what a guided step costs next to an unguided step of the same
backbone rows.

    python tools/guidance_bench.py [--steps 20] [--warmup 5] [--repeats 3]
    python tools/guidance_bench.py --summarize-trace DIR     (DIR: a rocprofv3 --kernel-trace --stats run of this tool)

The pair of bench.py's imagenet256 workload (uvit_imagenet256_3 -> uvit_imagenet256, synthetic weights, bf16, hipGraph replay, the
30 / 70 shallow / full mix, device Philox noise), built ONCE with max_batch 64, runs
  guided    B = 32 images, scale 0.4, null label 1000  (64 backbone rows per step)
  unguided  B = 64 images                              (64 backbone rows per step)
alternating, `repeats` times each, each run timed by hipEvents on its stream.  The backbone work of the two is identical; only
the step's last kernel differs (final_tiled_kernel<4, 2, true> over 32 images reading 64 images' decoder rows and writing 64
images of x, against final_tiled_kernel<4, 2, false> over 64 images).  Writes profiles/guidance/guidance_bench.json.
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

OUT = REPO / "profiles" / "guidance"
SCALE, NULL = 0.4, 1000


def bench(a):
    import torch
    from duodiff_amd import _lib
    from duodiff_amd.engine import sample_loop

    if not torch.cuda.is_available():
        raise SystemExit("guidance_bench.py needs an MI355X: the engine has no CPU path")
    dev = "cuda:0"
    torch.cuda.set_device(0)
    rows = 64
    es, ef, _, mp_f = synthetic_pair("uvit_imagenet256_3.yaml", "uvit_imagenet256.yaml", (1237, 1236), rows)
    ctx = es.ctx
    K, W = a.steps, a.warmup
    k_sw = max(1, round(0.3 * K))          # the 30 / 70 mix: the switch after 30 % of the steps
    g = torch.Generator().manual_seed(0)
    S, Cc = mp_f.img_size, mp_f.in_chans
    cases = {
        "guided_B32": dict(B=32, guidance=(SCALE, NULL)),
        "unguided_B64": dict(B=64, guidance=None),
    }
    state = {}
    for name, c in cases.items():
        x_T = torch.randn(c["B"], Cc, S, S, generator=g).to(dev)
        y = torch.randint(0, 1000, (c["B"],), generator=g).to(dev)       # every image guided (no label equals the null label)
        state[name] = (x_T, x_T.clone(), y)
    timer = LoopTimer(ctx)

    def run(name, k, ksw, timed):
        x_T, x, y = state[name]
        return timer.run(lambda stream: sample_loop(ctx, es, ef, x, t_switch=ksw, t_start=999, t_end=1000 - k, y=y, seed=0, noise="philox",
                                                    use_graph=True, stream=stream, guidance=cases[name]["guidance"]), x, x_T, name, timed=timed)

    for name in cases:                     # warm-up: both backbones of both cases (graph captures, code-object loads)
        if W > 0:
            run(name, W, max(1, W // 2), False)
    res = {name: {"ms_per_step": [], "images_per_s": []} for name in cases}
    chains = {}
    for r in range(a.repeats):
        for name, c in cases.items():
            ms, chains[name] = run(name, K, k_sw, True)
            res[name]["ms_per_step"].append(ms / K)
            res[name]["images_per_s"].append(c["B"] / (ms / K))    # a 1000-step sample takes ms_per_step seconds
            print(f"repeat {r} {name}: {ms / K:.3f} ms/step, {c['B'] / (ms / K):.3f} images/s, chains {chains[name]}", flush=True)
    out = {"_build_id": _lib.load().dd_build_id().decode(),
           "config": {"pair": "uvit_imagenet256_3 (first 30 % of the steps) -> uvit_imagenet256", "precision": "bf16", "hipgraph": True,
                      "noise": "device Philox", "weights": "synthetic (bench.py seeds)", "max_batch": rows, "steps_per_run": K,
                      "switch_after_steps": k_sw, "warmup_steps": W, "repeats": a.repeats, "order": "alternating guided / unguided",
                      "guidance": {"scale": SCALE, "null_label": NULL}, "timing": "hipEvents around each dd_sample call on its stream",
                      "date": time.strftime("%Y-%m-%d")}}
    for name, c in cases.items():
        out[name] = {"B_images": c["B"], "backbone_rows": rows, "chains": chains[name],
                     "ms_per_step": spread(res[name]["ms_per_step"]), "images_per_s": spread(res[name]["images_per_s"])}
    out["guided_over_unguided_ms_per_step"] = out["guided_B32"]["ms_per_step"]["median"] / out["unguided_B64"]["ms_per_step"]["median"]
    out["target"] = "guided B=32 ms/step <= 1.05 x unguided B=64 ms/step"
    out["target_met"] = out["guided_over_unguided_ms_per_step"] <= 1.05
    print(json.dumps(out, indent=1))
    if not a.no_json:
        OUT.mkdir(parents=True, exist_ok=True)
        (OUT / "guidance_bench.json").write_text(json.dumps(out, indent=1) + "\n")


def summarize_trace(d):
    """Mean / median duration per launch of the guided and unguided final kernels from a kernel trace of this tool."""
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
           "source": "rocprofv3 --kernel-trace --stats of tools/guidance_bench.py (its own run); durations in microseconds",
           "note": "both cases run as two chains: a guided launch covers 16 images (32 images of decoder rows, 32 of x written), an "
                   "unguided launch 32 images", "kernels": {}}
    for n, v in sorted(durs.items()):
        out["kernels"][n] = {"launches": len(v), "mean_us": statistics.mean(v), "median_us": statistics.median(v), "min_us": min(v)}
    g = [k for k in out["kernels"] if "true" in k or "Lb1E" in k]
    u = [k for k in out["kernels"] if "false" in k or "Lb0E" in k]
    if len(g) == 1 and len(u) == 1:
        out["guided_over_unguided_median"] = out["kernels"][g[0]]["median_us"] / out["kernels"][u[0]]["median_us"]
        out["target"] = "guided final kernel <= 1.10 x the unguided final kernel at 2B images"
        out["target_met"] = out["guided_over_unguided_median"] <= 1.10
    print(json.dumps(out, indent=1))
    OUT.mkdir(parents=True, exist_ok=True)
    (OUT / "final_kernel_trace.json").write_text(json.dumps(out, indent=1) + "\n")


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
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
