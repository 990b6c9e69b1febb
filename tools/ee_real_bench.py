"""Real early exit against the simulated early-exit loop: what a threshold buys in time.

    python tools/ee_real_bench.py [--steps 100] [--repeats 5]

The CelebA early-exit model (configs/deediff_celeba.yaml, depth 13; synthetic weights, bf16, device Philox), B = 128, the first `steps`
DDPM steps.  The simulated loop (dd_sample_early_exit: hipGraph replay, two half-batch chains, every image runs every block) and the real
loop (dd_sample_early_exit_real: eager launches, the host waits at every compaction layer) alternate in one process, `repeats` times each
per setting; medians, each run timed by hipEvents around the call on its stream.
Thresholds: +inf (every image leaves at layer 0), two found by bisection on the simulated loop's own idx table so that the mean exit
layer is about depth / 4 and depth / 2, and one below every prediction (nobody leaves).  compact_every in {1, 2, 4}.
With synthetic weights the exit distribution is not a trained model's: the table says what a given distribution of exits costs, not
which one a checkpoint yields.  Image quality is unchanged by construction (the loops agree bit for bit; the tool checks it).
Writes profiles/ee_real/ee_real_bench.json.
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

OUT = REPO / "profiles" / "ee_real"
B, SEED = 128, 1234


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    from duodiff_amd import _lib
    from duodiff_amd.config import ModelParams, load_config
    from duodiff_amd.early_exit import EarlyExitUViT, real_exit_block_rows
    from duodiff_amd.engine import real_exit_stats, sample_early_exit_loop, sample_early_exit_real_loop
    from duodiff_amd.uvit import UViT
    from duodiff_amd.weights import synthetic_ee_state_dict
    if not torch.cuda.is_available():
        raise SystemExit("ee_real_bench.py needs an MI355X: the engine has no CPU path")
    torch.cuda.set_device(0)
    mpd = dict(load_config(REPO / "configs" / "deediff_celeba.yaml")["model_params"])
    ctype = mpd.pop("classifier_type")
    mp = ModelParams.from_dict(mpd)
    m = EarlyExitUViT(UViT(**mp.as_dict(), precision="bf16", max_batch=B), ctype)
    m.load_state_dict(synthetic_ee_state_dict(mp, SEED, ctype)).eval().to("cuda")
    em = m.engine_model(B)
    ctx = em.ctx
    depth, steps = mp.depth, a.steps
    x_T = torch.randn(B, mp.in_chans, mp.img_size, mp.img_size, generator=torch.Generator().manual_seed(0)).cuda()
    stream = torch.cuda.Stream()
    idx = torch.zeros(1000, B, device="cuda", dtype=torch.int32)

    def run(thr, s=None):
        """one loop call -> (ms, x, idx rows); s None: the simulated loop"""
        x = x_T.clone()
        idx.zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            if s is None:
                sample_early_exit_loop(ctx, em, x, thr, t_start=999, t_end=1000 - steps, seed=SEED, idx=idx, stream=stream)
            else:
                sample_early_exit_real_loop(ctx, em, x, thr, t_start=999, t_end=1000 - steps, seed=SEED, idx=idx, compact_every=s, stream=stream)
            e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), x, idx[1000 - steps:].clone()

    def mean_exit(thr):
        return float(run(thr)[2].float().mean())

    def bisect(target):
        lo, hi = 0.0, 1.0            # an MLP probe's prediction is a mean of sigmoids; the mean exit layer falls as the threshold rises
        for _ in range(14):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if mean_exit(mid) > target else (lo, mid)
        return hi

    run(0.5), run(0.5, 1)                                    # captures, allocations
    thresholds = {"all_leave_at_0": float("inf"), "mean_exit_depth_4": bisect(depth / 4), "mean_exit_depth_2": bisect(depth / 2),
                  "nobody_leaves": 1e-30}
    out = {"_build_id": _lib.load().dd_build_id().decode(),
           "config": {"model": "deediff_celeba.yaml", "depth": depth, "B": B, "precision": "bf16", "steps": steps, "noise": "device Philox",
                      "weights": "synthetic (the exit distribution is not a trained model's)", "repeats": a.repeats,
                      "order": "simulated and real loops alternate within a threshold", "timing": "hipEvents around each loop call on its stream",
                      "simulated": "dd_sample_early_exit, hipGraph replay, two half-batch chains",
                      "real": "dd_sample_early_exit_real, eager launches, two half-batch chains", "date": time.strftime("%Y-%m-%d")},
           "rows": []}
    for name, thr in thresholds.items():
        ms = {None: [], 1: [], 2: [], 4: []}
        info = {}
        for _ in range(a.repeats):
            t_sim, x_sim, i_sim = run(thr)
            ms[None].append(t_sim)
            for s in (1, 2, 4):
                t, x, i = run(thr, s)
                ms[s].append(t)
                assert torch.equal(x, x_sim) and torch.equal(i, i_sim), f"{name} compact_every {s}: the real loop disagrees with the simulated one"
                rows, moves, compactions = real_exit_stats(ctx)
                wait, waits, moved = C.c_double(), C.c_longlong(), C.c_longlong()
                ctx.check(ctx.lib.dd_dev_ee_real_cost(ctx.handle, C.byref(wait), C.byref(waits), C.byref(moved)))
                info[s] = dict(block_rows=rows, moves=moves, compactions=compactions, host_wait_ms=wait.value, host_waits=waits.value,
                               bytes_moved=moved.value)
        sim = statistics.median(ms[None]) / steps
        row = {"threshold": name, "value": thr if thr != float("inf") else "inf", "mean_exit_layer": float(i_sim.float().mean()), "simulated_ms_per_step": sim,
               "simulated_spread": [min(ms[None]) / steps, max(ms[None]) / steps], "real": {}}
        for s in (1, 2, 4):
            r = statistics.median(ms[s]) / steps
            d = info[s]
            assert thr < 0 or d["block_rows"] == real_exit_block_rows(i_sim.cpu(), depth, s)
            row["real"][f"compact_every_{s}"] = {
                "ms_per_step": r, "spread": [min(ms[s]) / steps, max(ms[s]) / steps], "ratio_to_simulated": r / sim,
                "block_rows_share": d["block_rows"] / (steps * B * depth), "moves_per_step": d["moves"] / steps, "mbytes_moved_per_step": d["bytes_moved"] / steps / 1e6,
                "compactions_per_step": d["compactions"] / steps, "host_waits_per_step": d["host_waits"] / steps,
                "host_wait_us_per_wait": 1000.0 * d["host_wait_ms"] / max(d["host_waits"], 1)}
        out["rows"].append(row)
        print(json.dumps(row), flush=True)
    top = out["rows"][0]
    out["expectation"] = {"all_leave_at_0_real_faster_than_simulated": all(v["ratio_to_simulated"] < 1.0 for v in top["real"].values())}
    OUT.mkdir(parents=True, exist_ok=True)
    (OUT / "ee_real_bench.json").write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out["expectation"]))
    assert out["expectation"]["all_leave_at_0_real_faster_than_simulated"], "threshold +inf: the real loop must beat the simulated loop"


if __name__ == "__main__":
    main()
