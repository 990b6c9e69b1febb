"""Perturbed-attention guidance on the CelebA-64 pair: what a PAG step costs next to an unguided step of the same backbone rows, and
the identity-attention launch next to the attention launch it stands in for.

    python tools/pag_bench.py [--steps 20] [--warmup 5] [--repeats 5]
    python tools/pag_bench.py --kernel [--iters 50]

Default: the pair of bench.py's headline workload (uvit_celeba_3 -> uvit_celeba, synthetic weights, bf16, hipGraph replay, the
30 / 70 shallow / full mix, device Philox noise), built ONCE with max_batch 128, runs
  pag_mid   B = 64 images, scale 3.0, mask {mid} of either model    (128 backbone rows per step)
  pag_all   B = 64 images, scale 3.0, every block of either model   (128 backbone rows per step)
  unguided  B = 128 images                                          (128 backbone rows per step)
alternating, `repeats` times each, each run timed by hipEvents on its stream.  A PAG step replaces the attention of the masked blocks
on half of the rows by the lighter identity launch, so it must not be slower than the unguided step by more than the min-max spread of
the alternated unguided runs.
--kernel: dd_dev_v_identity and dd_dev_qkv_attention_rows at B = 64, embed_dim 512, one extra token, timed by the harness (events around
`iters` launches), alternating, `repeats` times each; the identity launch's share of the HBM rate over its algorithmic traffic (rows in
+ rows out).  Either mode merges its results into profiles/pag/pag_bench.json.
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

OUT = REPO / "profiles" / "pag"
SCALE = 3.0
HBM_ACHIEVABLE_TBS = 6.3        # a float4 copy on the MI355X (8.0 TB/s spec)


def bench(a):
    import torch
    from duodiff_amd import _lib
    from duodiff_amd.engine import Perturbed, sample_loop

    if not torch.cuda.is_available():
        raise SystemExit("pag_bench.py needs an MI355X: the engine has no CPU path")
    dev = "cuda:0"
    torch.cuda.set_device(0)
    rows = 128
    es, ef, mp_s, mp_f = synthetic_pair("uvit_celeba_3.yaml", "uvit_celeba.yaml", (1237, 1236), rows)
    ctx = es.ctx
    K, W = a.steps, a.warmup
    k_sw = max(1, round(0.3 * K))          # the 30 / 70 mix: the switch after 30 % of the steps
    g = torch.Generator().manual_seed(0)
    S, Cc = mp_f.img_size, mp_f.in_chans
    cases = {
        "pag_mid_B64": dict(B=64, guidance=Perturbed(SCALE, [mp_s.depth // 2], [mp_f.depth // 2])),
        "unguided_B128": dict(B=128, guidance=None),
        "pag_all_B64": dict(B=64, guidance=Perturbed(SCALE, list(range(mp_s.depth)), list(range(mp_f.depth)))),
    }
    state = {}
    for name, c in cases.items():
        x_T = torch.randn(c["B"], Cc, S, S, generator=g).to(dev)
        state[name] = (x_T, x_T.clone())
    timer = LoopTimer(ctx)

    def run(name, k, ksw, timed):
        x_T, x = state[name]
        return timer.run(lambda stream: sample_loop(ctx, es, ef, x, t_switch=ksw, t_start=999, t_end=1000 - k, seed=0, noise="philox",
                                                    use_graph=True, stream=stream, guidance=cases[name]["guidance"]), x, x_T, name, timed=timed)

    for name in cases:                     # warm-up: both backbones of every case (graph captures, code-object loads)
        if W > 0:
            run(name, W, max(1, W // 2), False)
    res = {name: [] for name in cases}
    chains = {}
    for r in range(a.repeats):
        for name in cases:
            ms, chains[name] = run(name, K, k_sw, True)
            res[name].append(ms / K)
            print(f"repeat {r} {name}: {ms / K:.3f} ms/step, chains {chains[name]}", flush=True)
    out = {"_build_id": _lib.load().dd_build_id().decode(),
           "config": {"pair": "uvit_celeba_3 (first 30 % of the steps) -> uvit_celeba", "precision": "bf16", "hipgraph": True,
                      "noise": "device Philox", "weights": "synthetic (bench.py seeds)", "max_batch": rows, "steps_per_run": K,
                      "switch_after_steps": k_sw, "warmup_steps": W, "repeats": a.repeats, "order": "alternating pag_mid / unguided / pag_all",
                      "scale": SCALE, "timing": "hipEvents around each loop call on its stream", "date": time.strftime("%Y-%m-%d")}}
    for name, c in cases.items():
        out[name] = {"B_images": c["B"], "backbone_rows": rows, "chains": chains[name], "ms_per_step": spread(res[name])}
    un = out["unguided_B128"]["ms_per_step"]
    allowed = un["median"] + (un["max"] - un["min"])
    for name in ("pag_mid_B64", "pag_all_B64"):
        med = out[name]["ms_per_step"]["median"]
        out[name]["over_unguided_ms_per_step"] = med / un["median"]
        out[name]["not_slower_than_unguided_plus_its_spread"] = med <= allowed
    out["target"] = "PAG B=64 ms/step <= unguided B=128 ms/step + the min-max spread of the alternated unguided runs"
    print(json.dumps(out, indent=1))
    if not a.no_json:
        merge_json(OUT / "pag_bench.json", {"loop": out})


def kernel(a):
    import numpy as np
    import torch
    from duodiff_amd import _lib
    from duodiff_amd.engine import Context

    if not torch.cuda.is_available():
        raise SystemExit("pag_bench.py needs an MI355X: the engine has no CPU path")
    ctx = Context.get()
    B, H, E = 64, 8, 1
    D, L_ = 64 * H, 256 + E
    r = np.random.default_rng(0)
    h = r.standard_normal((B * L_, D), dtype=np.float32)
    w = (r.standard_normal((3 * D, D)) / np.sqrt(D)).astype(np.float32)
    xres = r.standard_normal((B * L_, D), dtype=np.float32)
    ln = np.ascontiguousarray(np.stack([1.0 + 0.2 * r.standard_normal(D), 0.3 * r.standard_normal(D)]), np.float32)
    out = np.zeros((B * L_ + 8, D), np.uint16)
    entries = {"v_identity": ctx.lib.dd_dev_v_identity, "qkv_attention": ctx.lib.dd_dev_qkv_attention_rows}
    us = {name: [] for name in entries}
    for rep in range(a.repeats + 1):          # the first round warms both launches up
        for name, fn in entries.items():
            ms = C.c_float(0)
            ctx.check(fn(ctx.handle, B, L_, H, E, h.ctypes.data, w.ctypes.data, None, xres.ctypes.data, ln.ctypes.data, out.ctypes.data,
                         a.iters, None, C.byref(ms)))
            if rep:
                us[name].append(ms.value * 1e3)
                print(f"repeat {rep - 1} {name}: {ms.value * 1e3:.1f} us / launch", flush=True)
    traffic = 2 * B * L_ * D * 2            # rows in (norm1 as bf16; the extra rows' fp32 source is 0.4 % more) + rows out
    res = {"_build_id": _lib.load().dd_build_id().decode(),
           "config": {"B": B, "embed_dim": D, "extras": E, "iters_per_timing": a.iters, "repeats": a.repeats,
                      "timing": "the dev harness: events around `iters` back-to-back launches; alternating the two launches",
                      "date": time.strftime("%Y-%m-%d")},
           "v_identity_us": spread(us["v_identity"]), "qkv_attention_us": spread(us["qkv_attention"]),
           "algorithmic_traffic_bytes": traffic, "flop": 2 * B * L_ * D * D}
    med = res["v_identity_us"]["median"]
    res["v_identity_tb_per_s"] = traffic / (med * 1e-6) / 1e12
    res["v_identity_fraction_of_achievable_hbm"] = res["v_identity_tb_per_s"] / HBM_ACHIEVABLE_TBS
    res["note"] = ("back-to-back launches on the same 33 MB: the operands fit the 256 MB Infinity Cache, so the rate is an upper estimate of what "
                   "the launch reaches inside a step, where other launches' traffic lies between two of its runs")
    res["v_identity_over_qkv_attention"] = med / res["qkv_attention_us"]["median"]
    print(json.dumps(res, indent=1))
    if not a.no_json:
        merge_json(OUT / "pag_bench.json", {"kernel": res})


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--kernel", action="store_true", help="time the identity launch against the attention launch instead of the loops")
    p.add_argument("--no_json", action="store_true", help="print only")
    a = p.parse_args(argv)
    if a.kernel:
        kernel(a)
    else:
        bench(a)


if __name__ == "__main__":
    main()
