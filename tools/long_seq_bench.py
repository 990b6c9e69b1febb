"""What a long token sequence costs: the streaming attention launch beside the single-pass one, and a 1024-patch forward beside a 256-patch
forward of the same token count.  One process, one GPU; every figure is a median of repeated timed windows behind a discarded warm-up.

    python tools/long_seq_bench.py [--out profiles/long_seq/long_seq_bench.json] [--repeats 5] [--iters 1000]

Kernel times (the dev entry points' iters / ms_out: `iters` launches between two events on one stream), bf16, H = 8, B = 16:
    dd_dev_attention_long at L = 1025;  dd_dev_attention_long and dd_dev_attention at L = 288
    reported as us per launch and achieved TFLOP/s, counted as 4 L^2 64 per (image, head) -- the two matrix products, no softmax.
    The yardstick is the single-pass kernel's rate at L = 288 in the same run.
Forward times (events around `iters` forwards on a side stream), bf16, a synthetic CelebA-shaped model (embed_dim 512, depth 13, patch 4):
    img 128 at B = 16 (1025 tokens per image) beside img 64 at B = 64 (257 tokens per image): 16400 and 16448 token rows.
"""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

PREC_BF16 = 0


def spread(v):
    med = statistics.median(v)
    return {"runs": v, "median": med, "min": min(v), "max": max(v), "spread_frac": (max(v) - min(v)) / med if med else None}


def attention_flops(B, H, L):
    return 4.0 * L * L * 64 * B * H


def time_attention(ctx, entry, B, H, L, iters, repeats):
    """us per launch of one dev entry point: the first call (untimed launch + `iters` timed ones) is the warm-up and is discarded"""
    r = np.random.default_rng(L)
    q, k, v = (np.ascontiguousarray(r.standard_normal((B, H, L, 64)), np.float32) for _ in range(3))
    out = np.zeros((B * L + 8, 64 * H), np.uint16)
    fn = getattr(ctx.lib, entry)
    us = []
    for i in range(repeats + 1):
        ms = C.c_float(0)
        ctx.check(fn(ctx.handle, PREC_BF16, B, L, H, q.ctypes.data, k.ctypes.data, v.ctypes.data, out.ctypes.data, iters, None, C.byref(ms)))
        if i:
            us.append(1e3 * ms.value)          # ms_out is per launch
    rec = spread(us)
    rec.update(entry=entry, B=B, H=H, L=L, iters=iters, unit="us per launch", tflops=attention_flops(B, H, L) / (rec["median"] * 1e-6) / 1e12)
    return rec


def time_forward(img, B, iters, repeats):
    import torch
    from duodiff_amd.config import ModelParams
    from duodiff_amd.uvit import UViT
    from duodiff_amd.weights import synthetic_state_dict
    cfg = dict(img_size=img, patch_size=4, in_chans=3, embed_dim=512, depth=13, num_heads=8, mlp_ratio=4, qkv_bias=False,
               mlp_time_embed=False, num_classes=-1, normalize_timesteps=True)
    mp = ModelParams.from_dict(cfg)
    m = UViT(**mp.as_dict(), precision="bf16", max_batch=B).load_state_dict(synthetic_state_dict(mp, 7)).to("cuda:0")
    em = m.engine_model(B)
    x = torch.randn(B, 3, img, img, generator=torch.Generator().manual_seed(1)).cuda()
    out = torch.empty_like(x)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    with torch.cuda.stream(stream):
        for i in range(repeats + 1):            # window 0 is the warm-up
            e0.record(stream)
            for _ in range(iters):
                em.forward(x, 500.0, None, out=out, stream=stream)
            e1.record(stream)
            stream.synchronize()
            if i:
                ms.append(e0.elapsed_time(e1) / iters)
    assert torch.isfinite(out).all()
    rec = spread(ms)
    rec.update(img=img, B=B, tokens_per_image=(img // 4) ** 2 + 1, token_rows=B * ((img // 4) ** 2 + 1), iters=iters, unit="ms per forward")
    del em, m
    return rec


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default=str(REPO / "profiles" / "long_seq" / "long_seq_bench.json"))
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--iters", type=int, default=1000, help="launches per timed kernel window; a tenth as many forwards per forward window")
    a = p.parse_args(argv)
    import torch
    assert torch.cuda.is_available(), "long_seq_bench needs the MI355X: there is nothing to measure without it"
    from duodiff_amd.engine import Context
    ctx = Context.get()
    B, H = 16, 8
    res = {"kernels": {
        "long_1025": time_attention(ctx, "dd_dev_attention_long", B, H, 1025, a.iters, a.repeats),
        "long_288": time_attention(ctx, "dd_dev_attention_long", B, H, 288, a.iters, a.repeats),
        "single_pass_288": time_attention(ctx, "dd_dev_attention", B, H, 288, a.iters, a.repeats),
    }, "forwards": {
        "img128_B16": time_forward(128, 16, max(a.iters // 10, 1), a.repeats),
        "img64_B64": time_forward(64, 64, max(a.iters // 10, 1), a.repeats),
    }, "device": torch.cuda.get_device_name(0)}
    k = res["kernels"]
    res["long_1025_rate_over_single_pass_288_rate"] = k["long_1025"]["tflops"] / k["single_pass_288"]["tflops"]
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    for name, r in k.items():
        print(f"{name}: {r['median']:.1f} us ({r['min']:.1f} .. {r['max']:.1f}), {r['tflops']:.1f} TFLOP/s")
    for name, r in res["forwards"].items():
        print(f"{name}: {r['median']:.3f} ms per forward ({r['min']:.3f} .. {r['max']:.3f}), {r['token_rows']} token rows")
    print(json.dumps({"long_1025_rate_over_single_pass_288_rate": res["long_1025_rate_over_single_pass_288_rate"]}))


if __name__ == "__main__":
    main()
