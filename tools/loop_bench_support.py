"""What the A/B loop benches share (guidance_bench, autoguidance_bench, pag_bench, multistep_bench, threshold_bench): the statistics of a
series of runs, the synthetic shallow / full pair on the engine, one loop call timed by events on a side stream, a JSON record that several
modes of a tool write into."""
import json
import statistics
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
DEV = "cuda:0"


def spread(v):
    med = statistics.median(v)
    return {"runs": v, "median": med, "min": min(v), "max": max(v), "spread_frac": (max(v) - min(v)) / med if med else None}


def synthetic_pair(cfg_small, cfg_big, seeds, max_batch):
    """bf16 engine models of two configs/*.yaml (the shallow or guide model, the full one) with synthetic weights, and their ModelParams"""
    import torch
    from duodiff_amd.config import ModelParams, load_config
    from duodiff_amd.uvit import UViT
    from duodiff_amd.weights import synthetic_state_dict
    mps = [ModelParams.from_dict(load_config(REPO / "configs" / cfg)) for cfg in (cfg_small, cfg_big)]
    models = [UViT(**mp.as_dict(), precision="bf16", max_batch=max_batch).load_state_dict(synthetic_state_dict(mp, seed)).to(DEV)
              for mp, seed in zip(mps, seeds)]
    torch.cuda.synchronize()
    return (*(m.engine_model(max_batch) for m in models), *mps)


class LoopTimer:
    """a side stream and a pair of events; run(): one loop call from x_T, timed by the events"""

    def __init__(self, ctx):
        import torch
        self.ctx = ctx
        self.stream = torch.cuda.Stream(device=DEV)
        self.stream.wait_stream(torch.cuda.current_stream())
        self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def run(self, loop, x, x_T, what, h=None, timed=True):
        """x <- x_T (and h <- 0), loop(stream) between the two events, synchronise, x finite -> (ms or None, dd_dev_last_sample_chains)"""
        import torch
        with torch.cuda.stream(self.stream):
            x.copy_(x_T, non_blocking=True)
            if h is not None:
                h.zero_()
            if timed:
                self.e0.record(self.stream)
            loop(self.stream)
            if timed:
                self.e1.record(self.stream)
        self.stream.synchronize()
        assert torch.isfinite(x).all(), what
        return (self.e0.elapsed_time(self.e1) if timed else None), self.ctx.lib.dd_dev_last_sample_chains(self.ctx.handle)


def merge_json(path, update):
    path.parent.mkdir(parents=True, exist_ok=True)
    out = json.loads(path.read_text()) if path.exists() else {}
    out.update(update)
    path.write_text(json.dumps(out, indent=1) + "\n")
