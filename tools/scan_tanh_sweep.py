"""E_TANH: the largest |scan_tanh_abs(d) - tanh|d|| over every fp32 argument, from the numpy mirror on the CPU (no GPU).

    python tools/scan_tanh_sweep.py [--chunk 16777216] [--stride 1]

Sweeps the bit patterns of all fp32 values from 0 to the clamp in chunks (--stride 1: every one of them), then the tail behind the
clamp (every value there gives the clamp's value: the error is 1 - tanh at the clamp's side and falls from there), inf, and the negative
mirror of a sample.  Prints one JSON line: e_tanh, where it is taken, the largest result and the count.  The result goes into
scan_tanh_abs's comment (csrc/step_update.h), DESIGN section 7k and tests/scan_support.py E_TANH."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from duodiff_amd.threshold_scan import TANH_CLAMP, tanh_abs_f32  # noqa: E402


def sweep(chunk, stride):
    top = int(np.float32(TANH_CLAMP).view(np.uint32))
    worst, where, biggest, count = 0.0, 0.0, 0.0, 0
    for lo in range(0, top + 1, chunk * stride):
        bits = np.arange(lo, min(lo + chunk * stride, top + 1), stride, dtype=np.uint32)
        x = bits.view(np.float32)
        r = tanh_abs_f32(x)
        e = np.abs(r.astype(np.float64) - np.tanh(x.astype(np.float64)))
        i = int(e.argmax())
        if e[i] > worst:
            worst, where = float(e[i]), float(x[i])
        biggest = max(biggest, float(r.max()))
        count += len(bits)
        if not ((r >= 0).all() and (r <= 1).all()):
            raise SystemExit(f"result outside [0, 1] in the chunk at bit pattern {lo:#x}")
    tail = np.array([np.nextafter(TANH_CLAMP, np.float32(np.inf)), 11.0, 100.0, 1e30, np.inf], np.float32)
    e_tail = float(np.abs(tanh_abs_f32(tail).astype(np.float64) - 1.0).max())       # (float64 tanh is 1 - 4e-9 at most there)
    e_tail += 1.0 - float(np.tanh(np.float64(TANH_CLAMP)))
    neg = -np.linspace(0, 12, 100001).astype(np.float32)
    assert (tanh_abs_f32(neg).view(np.uint32) == tanh_abs_f32(-neg).view(np.uint32)).all()
    assert tanh_abs_f32(np.float32(0)) == 0
    return {"e_tanh": max(worst, e_tail), "at": where, "e_tail": e_tail, "largest_result": biggest, "values": count, "stride": stride,
            "clamp": float(TANH_CLAMP)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunk", type=int, default=1 << 24)
    ap.add_argument("--stride", type=int, default=1)
    a = ap.parse_args()
    print(json.dumps(sweep(a.chunk, a.stride)))
