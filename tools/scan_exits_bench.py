"""The early-exit scan on deediff_celeba: what a scan step costs next to a step of the early-exit sampling loop of the same model, and
the exits kernel alone against the same work as one dd_dev_scan_error launch per exit.

    python tools/scan_exits_bench.py [--steps 20] [--warmup 5] [--repeats 5] [--iters 50]

deediff_celeba (synthetic weights, bf16, hipGraph replay, two half-batch chains, device Philox noise) at B = 128, built ONCE, runs
  scan     `steps` rows of dd_scan_error_early_exit (predict_noise, timesteps spread over 999 .. 0)
  sample   `steps` steps of dd_sample_early_exit from t = 999 (threshold 0.1; the loop whose step this change leaves as it is)
alternating, `repeats` times each, each run timed by hipEvents on its stream.  A scan step is the sampling step's forward between the
diffuse kernel and the exits kernel instead of in front of the select / step launch, so it should sit near the sampling step plus the two
scan kernels' stand-alone times.  The exits kernel is timed through dd_dev_scan_exits_error on one chain's share (64 images, depth + 1 =
14 exits: events around `iters` launches), next to diffuse and to 14 launches of dd_dev_scan_error on the same planes (the sum of their
stand-alone times), alternating, `repeats` times each.  Results go to profiles/scan/scan_exits_bench.json.
"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

from loop_bench_support import DEV, LoopTimer, merge_json, spread  # noqa: E402

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
    from duodiff_amd.config import ModelParams, load_config
    from duodiff_amd.early_exit import EarlyExitUViT
    from duodiff_amd.engine import sample_early_exit_loop, scan_exits_loop
    from duodiff_amd.step_plan import scan_rows
    from duodiff_amd.uvit import UViT
    from duodiff_amd.weights import synthetic_ee_state_dict

    if not torch.cuda.is_available():
        raise SystemExit("scan_exits_bench.py needs an MI355X: the engine has no CPU path")
    torch.cuda.set_device(0)
    B = 128
    config = load_config(REPO / "configs" / "deediff_celeba.yaml")
    ctype = config["model_params"]["classifier_type"]
    mp = ModelParams.from_dict(config)
    model = EarlyExitUViT(UViT(**mp.as_dict(), precision="bf16", max_batch=B), ctype)
    model.load_state_dict(synthetic_ee_state_dict(mp, 1236, ctype))
    em = model.eval().to(DEV).engine_model(B)
    ctx = em.ctx
    K, W = a.steps, a.warmup
    S, Cc, E = mp.img_size, mp.in_chans, mp.depth + 1
    g = torch.Generator().manual_seed(0)
    x0 = (torch.rand(B, Cc, S, S, generator=g) * 2 - 1).to(DEV).contiguous()
    x_T = torch.randn(B, Cc, S, S, generator=g).to(DEV)
    x = x_T.clone()
    timer = LoopTimer(ctx)
    last = {}

    def rows(k):
        return scan_rows(np.unique(np.linspace(999, 0, k).round().astype(int))[::-1], "predict_noise")

    def run(name, k, timed):
        if name == "sample":
            return timer.run(lambda st: sample_early_exit_loop(ctx, em, x, 0.1, t_start=999, t_end=1000 - k, seed=0, noise="philox", use_graph=True,
                                                               stream=st), x, x_T, name, timed=timed)
        r = rows(k)
        assert len(r["t"]) == k
        return timer.run(lambda st: last.__setitem__("scan", scan_exits_loop(ctx, em, x0, r, seed=0, use_graph=True, stream=st)), x0, x0, name, timed=timed)

    for name in ("scan", "sample"):          # warm-up: graph captures, code-object loads
        if W > 0:
            run(name, W, False)
    res, chains = {"scan": [], "sample": []}, {}
    for rep in range(a.repeats):
        for name in ("scan", "sample"):
            ms, chains[name] = run(name, K, True)
            res[name].append(ms / K)
            print(f"repeat {rep} {name}: {ms / K:.3f} ms/step, chains {chains[name]}", flush=True)
    assert all(torch.isfinite(t).all() for t in last["scan"])

    # the kernels alone on one chain's share: 64 images, 14 exits
    nb = B // 2
    x0h = x0[:nb].cpu().numpy()
    planes = np.random.default_rng(1).standard_normal((E, nb, Cc, S, S)).astype(np.float32)
    cls = np.random.default_rng(2).uniform(0, 1, (E - 1, nb)).astype(np.float32)
    us = {}
    for rep in range(a.repeats + 1):          # the first round warms every launch up
        q = _lib.dd_dev_scan_exits_args()
        q.B, q.C, q.S, q.exits, q.b0, q.B_all, q.k, q.t, q.next = nb, Cc, S, E, 0, nb, 0, 500, 499
        q.t_model, q.ka, q.kb, q.tz, q.t0, q.tx, q.ctr, q.seed, q.iters = 500.0, 0.28, 0.96, 1.0, 0.0, 0.0, 0, 1, a.iters
        o = [np.zeros(E * nb + 8, np.float32), np.zeros(E * nb + 8, np.float32), np.zeros((E - 1) * nb + 8, np.float32)]
        ctx.check(ctx.lib.dd_dev_scan_exits_error(ctx.handle, C.byref(q), x0h.ctypes.data, planes[:-1].ctypes.data, planes[-1].ctypes.data,
                                                  cls.ctypes.data, None, 0, o[0].ctypes.data, o[1].ctypes.data, o[2].ctypes.data, None))
        total = 0.0
        for l in range(E):
            d = _lib.dd_dev_scan_args()
            d.B, d.C, d.S, d.b0, d.B_all, d.k = nb, Cc, S, 0, nb, 0
            d.t_model, d.ka, d.kb, d.tz, d.t0, d.tx, d.ctr, d.seed, d.iters = 500.0, 0.28, 0.96, 1.0, 0.0, 0.0, 0, 1, a.iters
            out = np.zeros(nb + 8, np.float32)
            ctx.check(ctx.lib.dd_dev_scan_error(ctx.handle, C.byref(d), x0h.ctypes.data, planes[l].ctypes.data, None, 0, out.ctypes.data, None))
            total += d.ms_out * 1e3
            assert np.array_equal(out[:nb], o[0][l * nb:(l + 1) * nb])       # the same numbers, bit for bit
        f = _lib.dd_dev_scan_args()
        f.B, f.C, f.S, f.b0, f.B_all, f.k = nb, Cc, S, 0, nb, 0
        f.t_model, f.ka, f.kb, f.tz, f.t0, f.tx, f.ctr, f.seed, f.iters = 500.0, 0.28, 0.96, 1.0, 0.0, 0.0, 0, 1, a.iters
        xt = np.zeros(nb * Cc * S * S + 16, np.float32)
        ctx.check(ctx.lib.dd_dev_scan_diffuse(ctx.handle, C.byref(f), x0h.ctypes.data, None, 0, xt.ctypes.data, None))
        if rep:
            us.setdefault("exits_error", []).append(q.ms_out * 1e3)
            us.setdefault("scan_error_x14", []).append(total)
            us.setdefault("diffuse", []).append(f.ms_out * 1e3)
    read_bytes = (E + 1) * nb * Cc * S * S * 4          # the planes and x0, each read once
    out = {"_build_id": _lib.load().dd_build_id().decode(),
           "config": {"model": "deediff_celeba", "classifier_type": ctype, "precision": "bf16", "hipgraph": True, "noise": "device Philox",
                      "weights": "synthetic", "B": B, "steps_per_run": K, "warmup_steps": W, "repeats": a.repeats,
                      "order": "alternating scan / sample", "sampling_threshold": 0.1,
                      "timing": "hipEvents around each loop call on its stream; the kernels: events around `iters` launches of the dev entry",
                      "iters_per_kernel_timing": a.iters, "date": time.strftime("%Y-%m-%d")},
           "scan_ms_per_step": spread(res["scan"]), "sample_ms_per_step": spread(res["sample"]), "chains": chains,
           "kernels_us": {k: spread(v) for k, v in us.items()}, "kernel_shape": {"B": nb, "C": Cc, "S": S, "exits": E}}
    ex = out["kernels_us"]["exits_error"]["median"]
    out["exits_error_read_GBps"] = read_bytes / (ex * 1e-6) / 1e9
    out["exits_error_over_scan_error_x14"] = ex / out["kernels_us"]["scan_error_x14"]["median"]
    out["scan_minus_sample_ms"] = out["scan_ms_per_step"]["median"] - out["sample_ms_per_step"]["median"]
    out["two_scan_kernels_ms"] = (ex + out["kernels_us"]["diffuse"]["median"]) / 1e3
    out["note"] = ("the kernels of a chain (64 images) are timed alone, back to back on the same buffers: an upper estimate of their rate, a lower "
                   "one of their cost inside a step; the sampling step's select / step launch is not timed alone")
    print(json.dumps(out, indent=1))
    if not a.no_json:
        merge_json(OUT / "scan_exits_bench.json", out)


if __name__ == "__main__":
    main()
