"""Autoguidance: what an autoguided step of the full backbone costs next to the two unguided steps it is made of.

    python tools/autoguidance_bench.py [--steps 20] [--warmup 5] [--repeats 5]
    python tools/autoguidance_bench.py --trace-case auto|cfg                   (the run to put under rocprofv3 --kernel-trace --stats)
    python tools/autoguidance_bench.py --summarize-trace DIR --label auto|cfg  (DIR: the output of such a run)

Two pairs, synthetic weights (bench.py's seeds), bf16, hipGraph replay, device Philox noise, two half-batch chains:
  celeba       uvit_celeba_3 (guide) / uvit_celeba (main), B = 128, unconditional
  imagenet256  uvit_imagenet256_3 (guide) / uvit_imagenet256 (main), B = 32, class-conditional
Per pair three loops of `steps` DDPM steps, alternating, `repeats` times each:
  autoguided_late    the main model guided by the guide at scale 1.0   (B guide rows + B main rows + one output head per step)
  unguided_late      the main model alone                              (an existing loop)
  unguided_shallow   the guide alone                                   (an existing loop)
The yardstick of the autoguided step is the SUM of the two unguided steps of the same process.  The time of a loop is
dd_last_sample_timing's (hipEvents on the stream around the replays: graph capture is outside).  Writes
profiles/autoguidance/autoguidance_bench.json; the trace summaries go to profiles/autoguidance/final_kernel_trace.json.
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

OUT = REPO / "profiles" / "autoguidance"
SCALE = 1.0
PAIRS = {"celeba": ("uvit_celeba_3", "uvit_celeba", 128), "imagenet256": ("uvit_imagenet256_3", "uvit_imagenet256", 32)}


def build_pair(name, max_batch):
    cfg_g, cfg_m, _ = PAIRS[name]
    eg, em, _, mp_m = synthetic_pair(f"{cfg_g}.yaml", f"{cfg_m}.yaml", (1237, 1236), max_batch)
    return eg, em, mp_m


def runner(eg, em, mp, B):
    """run(case, k) -> (ms of the loop's replays, chains); cases: autoguided_late, unguided_late, unguided_shallow, cfg_late"""
    import torch
    from duodiff_amd.engine import Autoguidance, sample_loop
    g = torch.Generator().manual_seed(0)
    x_T = torch.randn(B, mp.in_chans, mp.img_size, mp.img_size, generator=g).to("cuda:0")
    y = torch.randint(0, 1000, (B,), generator=g).to("cuda:0") if mp.num_classes > 0 else None
    x = x_T.clone()
    ctx = em.ctx
    timer = LoopTimer(ctx)

    def run(case, k):
        model = eg if case == "unguided_shallow" else em
        kw = {"autoguided_late": dict(guidance=Autoguidance(eg, SCALE)), "cfg_late": dict(guidance=(SCALE, 1000))}.get(case, {})
        _, chains = timer.run(lambda stream: sample_loop(ctx, model, None, x, t_start=999, t_end=1000 - k, y=y, seed=0, noise="philox",
                                                         use_graph=True, stream=stream, **kw), x, x_T, case, timed=False)
        return ctx.last_sample_timing()[0], chains      # the loop's own timing: graph capture is outside
    return run


def bench(a):
    import torch
    from duodiff_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("autoguidance_bench.py needs an MI355X: the engine has no CPU path")
    torch.cuda.set_device(0)
    K, W = a.steps, a.warmup
    cases = ("autoguided_late", "unguided_late", "unguided_shallow")
    out = {"_build_id": _lib.load().dd_build_id().decode(),
           "config": {"precision": "bf16", "hipgraph": True, "noise": "device Philox", "weights": "synthetic (bench.py seeds)",
                      "scale": SCALE, "steps_per_run": K, "warmup_steps": W, "repeats": a.repeats, "order": "alternating, in the order of `cases`",
                      "cases": list(cases), "timing": "dd_last_sample_timing[0]: hipEvents around the loop's replays on its stream",
                      "date": time.strftime("%Y-%m-%d")}}
    for pair, (_, _, B) in PAIRS.items():
        eg, em, mp = build_pair(pair, B)
        run = runner(eg, em, mp, B)
        for c in cases:
            if W > 0:
                run(c, W)
        ms = {c: [] for c in cases}
        chains = {}
        for r in range(a.repeats):
            for c in cases:
                t, chains[c] = run(c, K)
                ms[c].append(t / K)
                print(f"{pair} repeat {r} {c}: {t / K:.3f} ms/step, chains {chains[c]}", flush=True)
        res = {c: {"chains": chains[c], "ms_per_step": spread(ms[c])} for c in cases}
        med = {c: res[c]["ms_per_step"]["median"] for c in cases}
        yard = med["unguided_late"] + med["unguided_shallow"]
        # the run's own min-max spread of the yardstick: the two summands' spreads added
        yard_spread = sum(res[c]["ms_per_step"]["max"] - res[c]["ms_per_step"]["min"] for c in ("unguided_late", "unguided_shallow"))
        res.update(B_images=B, yardstick_ms_per_step=yard, yardstick_min_max_spread_ms=yard_spread,
                   autoguided_over_yardstick=med["autoguided_late"] / yard,
                   autoguided_minus_yardstick_ms=med["autoguided_late"] - yard,
                   autoguided_over_unguided_late=med["autoguided_late"] / med["unguided_late"],
                   expectation="autoguided_late <= unguided_late + unguided_shallow",
                   expectation_met=med["autoguided_late"] <= yard,
                   within_spread=med["autoguided_late"] - yard <= yard_spread)
        out[pair] = res
        del run, eg, em
    cfg = REPO / "profiles" / "guidance" / "guidance_bench.json"
    if cfg.exists():
        out["cfg_reference"] = {"source": "profiles/guidance/guidance_bench.json",
                                "guided_B32_over_unguided_B64_ms_per_step": json.loads(cfg.read_text())["guided_over_unguided_ms_per_step"],
                                "note": "a classifier-free guided step of B images costs that factor times an unguided step of 2 B rows"}
    print(json.dumps(out, indent=1))
    if not a.no_json:
        OUT.mkdir(parents=True, exist_ok=True)
        (OUT / "autoguidance_bench.json").write_text(json.dumps(out, indent=1) + "\n")


def trace_case(a):
    """The run for a kernel trace: the ImageNet-256 pair (max_batch 64 for both cases, so every launch in front of the output head is
    sized alike), B = 32 in two chains: an output-head launch covers 16 images, autoguided or classifier-free guided."""
    import torch
    torch.cuda.set_device(0)
    eg, em, mp = build_pair("imagenet256", 64)
    run = runner(eg, em, mp, 32)
    case = {"auto": "autoguided_late", "cfg": "cfg_late"}[a.trace_case]
    _, chains = run(case, a.warmup)
    ms, chains = run(case, a.steps)
    print(f"{case}: {ms / a.steps:.3f} ms/step, chains {chains}")


def summarize_trace(a):
    """Median duration per launch of the guided output-head kernel in a kernel trace of --trace-case, added to final_kernel_trace.json"""
    from duodiff_amd import _lib
    trace = glob.glob(os.path.join(a.trace, "**", "*kernel_trace.csv"), recursive=True)
    if not trace:
        raise SystemExit(f"no kernel_trace.csv under {a.trace}")
    durs = {}
    for f in trace:
        for r in csv.DictReader(open(f)):
            n = r["Kernel_Name"]
            if "final_tiled_kernel" in n:
                durs.setdefault(n, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    path = OUT / "final_kernel_trace.json"
    out = json.loads(path.read_text()) if path.exists() else {}
    out["_build_id"] = _lib.load().dd_build_id().decode()
    out["source"] = ("rocprofv3 --kernel-trace --stats of tools/autoguidance_bench.py --trace-case <label>, one run per label; ImageNet-256 "
                     "pair, B = 32 in two chains (16 images per output-head launch); durations in microseconds")
    out[a.label] = {n: {"launches": len(v), "mean_us": statistics.mean(v), "median_us": statistics.median(v), "min_us": min(v)}
                    for n, v in sorted(durs.items())}
    guided = lambda d: [v for k, v in d.items() if ", true," in k]
    if "auto" in out and "cfg" in out and len(guided(out["auto"])) == 1 and len(guided(out["cfg"])) == 1:
        out["autoguided_over_cfg_median"] = guided(out["auto"])[0]["median_us"] / guided(out["cfg"])[0]["median_us"]
    print(json.dumps(out, indent=1))
    OUT.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(out, indent=1) + "\n")


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--no_json", action="store_true", help="print only")
    p.add_argument("--trace-case", dest="trace_case", choices=["auto", "cfg"], default=None)
    p.add_argument("--summarize-trace", dest="trace", default=None)
    p.add_argument("--label", choices=["auto", "cfg"], default="auto")
    a = p.parse_args(argv)
    if a.trace:
        summarize_trace(a)
    elif a.trace_case:
        trace_case(a)
    else:
        bench(a)


if __name__ == "__main__":
    main()
