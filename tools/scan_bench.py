"""The denoising-error scan on the CelebA-64 full model: what a scan step costs next to a DDPM sampling step of the same model, and the
scan's two kernels alone.

    python tools/scan_bench.py [--steps 20] [--warmup 5] [--repeats 5] [--iters 50]

uvit_celeba (synthetic weights, bf16, hipGraph replay, two half-batch chains, device Philox noise) at B = 128, built ONCE, runs
  scan     `steps` rows of dd_scan_error (predict_noise, timesteps spread over 999 .. 0)
  sample   `steps` steps of dd_sample from t = 999 (the sampling loop, which the scan leaves untouched)
alternating, `repeats` times each, each run timed by hipEvents on its stream.  A scan step launches the forward of a sampling step
between its two kernels (the output head writes eps instead of the update), so it should sit within the sampling step's own min-max
spread plus the stand-alone times of the two kernels.  Those are timed through dd_dev_scan_diffuse / dd_dev_scan_error at the same shape
(events around `iters` launches), alternating, `repeats` times each.  Results go to profiles/scan/scan_bench.json.
"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

from loop_bench_support import LoopTimer, merge_json, spread, synthetic_pair  # noqa: E402

OUT = REPO / "profiles" / "scan"


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--no_json", action="store_true", help="print only")
    a = p.parse_args(argv)
    import numpy as np
    import torch
    from duodiff_amd import _lib
    from duodiff_amd.engine import sample_loop, scan_error_loop
    from duodiff_amd.step_plan import scan_rows

    if not torch.cuda.is_available():
        raise SystemExit("scan_bench.py needs an MI355X: the engine has no CPU path")
    torch.cuda.set_device(0)
    B = 128
    _, em, _, mp = synthetic_pair("uvit_celeba_3.yaml", "uvit_celeba.yaml", (1237, 1236), B)
    ctx = em.ctx
    K, W = a.steps, a.warmup
    S, Cc = mp.img_size, mp.in_chans
    g = torch.Generator().manual_seed(0)
    x0 = (torch.rand(B, Cc, S, S, generator=g) * 2 - 1).to("cuda:0").contiguous()
    x_T = torch.randn(B, Cc, S, S, generator=g).to("cuda:0")
    x = x_T.clone()
    timer = LoopTimer(ctx)
    err = {}

    def rows(k):
        return scan_rows(np.linspace(999, 0, k).round().astype(int), "predict_noise")

    def run(name, k, timed):
        if name == "sample":
            return timer.run(lambda st: sample_loop(ctx, em, None, x, t_start=999, t_end=1000 - k, seed=0, noise="philox", use_graph=True, stream=st),
                             x, x_T, name, timed=timed)
        r = rows(k)
        err[k] = torch.empty(k, B, device="cuda:0")
        return timer.run(lambda st: scan_error_loop(ctx, em, x0, r, seed=0, use_graph=True, stream=st, err=err[k]), x0, x0, name, timed=timed)

    for name in ("scan", "sample"):          # warm-up: graph captures, code-object loads
        if W > 0:
            run(name, W, False)
    res, chains = {"scan": [], "sample": []}, {}
    for rep in range(a.repeats):
        for name in ("scan", "sample"):
            ms, chains[name] = run(name, K, True)
            res[name].append(ms / K)
            print(f"repeat {rep} {name}: {ms / K:.3f} ms/step, chains {chains[name]}", flush=True)
    assert torch.isfinite(err[K]).all()

    # the two kernels alone at the loop's shape, one chain's share (64 images) and the whole batch
    x0h = x0.cpu().numpy()
    mh = np.random.default_rng(1).standard_normal(x0h.shape).astype(np.float32)
    us = {}
    for rep in range(a.repeats + 1):          # the first round warms both launches up
        for nb in (B // 2, B):
            for entry in ("diffuse", "error"):
                q = _lib.dd_dev_scan_args()
                q.B, q.C, q.S, q.b0, q.B_all, q.k = nb, Cc, S, 0, nb, 0
                q.t_model, q.ka, q.kb, q.tz, q.t0, q.tx, q.ctr, q.seed, q.iters = 500.0, 0.28, 0.96, 1.0, 0.0, 0.0, 0, 1, a.iters
                if entry == "diffuse":
                    out = np.zeros(nb * Cc * S * S + 16, np.float32)
                    ctx.check(ctx.lib.dd_dev_scan_diffuse(ctx.handle, C.byref(q), x0h.ctypes.data, None, 0, out.ctypes.data, None))
                else:
                    out = np.zeros(nb + 8, np.float32)
                    ctx.check(ctx.lib.dd_dev_scan_error(ctx.handle, C.byref(q), x0h.ctypes.data, mh.ctypes.data, None, 0, out.ctypes.data, None))
                if rep:
                    us.setdefault(f"{entry}_B{nb}", []).append(q.ms_out * 1e3)
    out = {"_build_id": _lib.load().dd_build_id().decode(),
           "config": {"model": "uvit_celeba", "precision": "bf16", "hipgraph": True, "noise": "device Philox", "weights": "synthetic (bench.py seeds)",
                      "B": B, "steps_per_run": K, "warmup_steps": W, "repeats": a.repeats, "order": "alternating scan / sample",
                      "timing": "hipEvents around each loop call on its stream; the kernels: events around `iters` launches of the dev entry",
                      "iters_per_kernel_timing": a.iters, "date": time.strftime("%Y-%m-%d")},
           "scan_ms_per_step": spread(res["scan"]), "sample_ms_per_step": spread(res["sample"]), "chains": chains,
           "kernels_us": {k: spread(v) for k, v in us.items()}}
    sm = out["sample_ms_per_step"]
    half = B // 2
    kernels_ms = (out["kernels_us"][f"diffuse_B{half}"]["median"] + out["kernels_us"][f"error_B{half}"]["median"]) / 1e3
    out["scan_over_sample"] = out["scan_ms_per_step"]["median"] / sm["median"]
    out["allowed_ms_per_step"] = sm["median"] + (sm["max"] - sm["min"]) + kernels_ms
    out["within_sample_spread_plus_the_two_kernels"] = out["scan_ms_per_step"]["median"] <= out["allowed_ms_per_step"]
    out["note"] = ("the two kernels of a chain (64 images) are timed alone, back to back on the same buffers: an upper estimate of their rate, "
                   "a lower one of their cost inside a step")
    print(json.dumps(out, indent=1))
    if not a.no_json:
        merge_json(OUT / "scan_bench.json", out)


if __name__ == "__main__":
    main()
