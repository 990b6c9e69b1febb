"""Shared by the tests of the two scans (test_scan_kernels.py, test_scan_loop.py, test_scan_exits_kernels.py, test_scan_exits_loop.py and,
on the CPU, test_switch_scan_cpu.py, test_threshold_scan_cpu.py): the rows, seeds and callers of the dev entries dd_dev_scan_diffuse /
dd_dev_scan_error / dd_dev_scan_exits_error with their float64 references, the measured constant of scan_tanh_abs, and the images and the
caller of the two device loops.  No GPU at import."""
import ctypes as C

import numpy as np
import torch

import kernel_support as ks
from duodiff_amd import _lib
from kernel_support import F32, U24, P
from loop_support import side_stream

PHILOX_SCAN = 0x7363616E
# target rows (tz, t0, tx) at (ka, kb) of a mid timestep: predict_noise, predict_original, predict_previous (values of t = 500)
KA, KB = F32(0.27892652), F32(0.96031439)
ROWS = {"predict_noise": (1.0, 0.0, 0.0), "predict_original": (0.0, 1.0, 0.0), "predict_previous": (0.0, 0.0080282, 0.9895465)}
SEED = (7 << 32) | 0x9ABCDEF1

# The largest |scan_tanh_abs(d) - tanh|d|| over every fp32 d against float64 tanh: tools/scan_tanh_sweep.py (all 1 092 616 193 values of
# [0, 10], the tail, inf), a CPU measurement of the numpy mirror duodiff_amd.threshold_scan.tanh_abs_f32.  The spec is <= 1e-6.
E_TANH = 1.66e-7                        # measured 1.6533e-7, at d = 1.1165210
TANH_BREAKPOINTS = (0.0, 10.0)          # the function's only breakpoints: |d| = 0 (the fabs) and the clamp


def _seeds(n):
    return (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(12345)).astype(np.uint64)


def _args(B, Cn, S, b0, B_all, k, ka, kb, row=(1.0, 0.0, 0.0), ctr=0, t_model=500.0, next_t_model=250.0, seed=SEED, advance=0):
    a = _lib.dd_dev_scan_args()
    a.B, a.C, a.S, a.b0, a.B_all, a.k = B, Cn, S, b0, B_all, k
    a.t_model, a.ka, a.kb, a.tz, a.t0, a.tx = t_model, ka, kb, *row
    a.ctr, a.next_t_model, a.seed, a.advance = ctr, next_t_model, seed, advance
    a.t_out = a.t_final_out = -12345
    a.t_model_out = -1.0
    return a


def diffuse(x0, b0, B_all, k=3, ka=KA, kb=KB, ctr=0, seeds=None, seed=SEED, expect=_lib.DD_OK):
    """dd_dev_scan_diffuse -> (x_t [B, C, S, S], the whole output buffer, the args read back)"""
    B, Cn, S, _ = x0.shape
    n = x0.size
    a = _args(B, Cn, S, b0, B_all, k, ka, kb, ctr=ctr, seed=seed)
    out = np.zeros(n + 16, F32)
    c = ks.ctx()
    rc = c.lib.dd_dev_scan_diffuse(c.handle, C.byref(a), P(np.ascontiguousarray(x0, F32)), P(seeds), 0 if seeds is None else len(seeds), P(out), None)
    assert rc == expect, (rc, c.lib.dd_last_error(c.handle))
    return out[8:8 + n].reshape(x0.shape), out, a


def error(x0, m, b0, B_all, row, k=3, ka=KA, kb=KB, ctr=0, seeds=None, seed=SEED, advance=0, expect=_lib.DD_OK):
    """dd_dev_scan_error -> (err [B], the whole err buffer, the args read back)"""
    B, Cn, S, _ = x0.shape
    a = _args(B, Cn, S, b0, B_all, k, ka, kb, row, ctr=ctr, seed=seed, advance=advance)
    out = np.zeros((k + 1) * B_all + 8, F32)
    c = ks.ctx()
    rc = c.lib.dd_dev_scan_error(c.handle, C.byref(a), P(np.ascontiguousarray(x0, F32)), P(np.ascontiguousarray(m, F32)), P(seeds),
                                 0 if seeds is None else len(seeds), P(out), None)
    assert rc == expect, (rc, c.lib.dd_last_error(c.handle))
    return out[k * B_all + b0:k * B_all + b0 + B].copy(), out, a


def draw(B, Cn, S, b0, B_all, ctr=0, seeds=None, seed=SEED):
    """the kernel's z: (ka, kb) = (0, 1) on x0 = 0 returns 0 * 0 + 1 * z"""
    return diffuse(np.zeros((B, Cn, S, S), F32), b0, B_all, ka=0.0, kb=1.0, ctr=ctr, seeds=seeds, seed=seed)[0]


def z_ref(B, Cn, S, b0, ctr, seeds, seed):
    """the host reference of the draw: draw_site's (key, id) -- plain: the call's seed and batch-wide pixel ids from b0; seeded: the image's
    own seed and image-local ids"""
    if seeds is None:
        return ks.final_philox_ref(seed, B, Cn, S, b0, ctr, PHILOX_SCAN)[0]
    return np.concatenate([ks.final_philox_ref(int(seeds[b0 + b]), 1, Cn, S, 0, ctr, PHILOX_SCAN)[0] for b in range(B)])


def error_ref(x0, m, z, ka, kb, row):
    """(err64 [B], bound [B], d [B, C, S, S]) from the fp32 operands: x_t in fp32 as the kernel forms it (bit-equal: the diffuse test), then float64"""
    B, Cn, S, _ = x0.shape
    xt = (F32(ka) * x0 + F32(kb) * z).astype(np.float64)
    tz, t0, tx = (float(F32(v)) for v in row)
    z64, x64 = z.astype(np.float64), x0.astype(np.float64)
    tgt = tz * z64 + t0 * x64 + tx * xt
    dt = 3 * U24 * (np.abs(tz * z64) + np.abs(t0 * x64) + np.abs(tx * xt))
    d = m.astype(np.float64) - tgt
    n = Cn * S * S
    depth = Cn * -(-S * S // 256) + 6 + 3                    # the summation depth scan_error_kernel states
    bound = ((depth + 4) * U24 * (d * d).sum((1, 2, 3)) + (2 * np.abs(d) * dt).sum((1, 2, 3))) / n
    return (d * d).sum((1, 2, 3)) / n, bound, d


def exits_args(B, Cn, S, exits, b0, B_all, k, t, nxt, ka, kb, row, ctr, t_model=500.0, next_t_model=250.0, seed=0, advance=0):
    a = _lib.dd_dev_scan_exits_args()
    a.B, a.C, a.S, a.exits, a.b0, a.B_all, a.k, a.t, a.next = B, Cn, S, exits, b0, B_all, k, t, nxt
    a.t_model, a.ka, a.kb, a.tz, a.t0, a.tx = t_model, ka, kb, *row
    a.ctr, a.next_t_model, a.seed, a.advance = ctr, next_t_model, seed, advance
    a.t_out = a.t_final_out = -12345
    a.t_model_out = -1.0
    return a


def exits_error(x0, planes, cls, b0, B_all, row, ka, kb, *, k=3, t=500, nxt=250, ctr=3, seeds=None, seed=0, advance=0, iters=0, expect=0):
    """dd_dev_scan_exits_error.  planes [E, B, C, S, S] (the last one is eps), cls [E - 1, B] -> dict(mse [E, B], tgtu [E, B], pred [E - 1, B],
    whole = the three whole buffers, args = the args read back)"""
    E, B, Cn, S, _ = planes.shape
    a = exits_args(B, Cn, S, E, b0, B_all, k, t, nxt, ka, kb, row, ctr, seed=seed, advance=advance)
    a.iters = iters
    mse, tgtu = (np.zeros((k + 1) * E * B_all + 8, F32) for _ in range(2))
    pred = np.zeros((k + 1) * (E - 1) * B_all + 8, F32)
    outs = np.ascontiguousarray(planes[:-1], F32) if E > 1 else None
    eps = np.ascontiguousarray(planes[-1], F32)
    clsc = np.ascontiguousarray(cls, F32) if E > 1 else None
    c = ks.ctx()
    rc = c.lib.dd_dev_scan_exits_error(c.handle, C.byref(a), P(np.ascontiguousarray(x0, F32)), P(outs), P(eps), P(clsc), P(seeds),
                                       0 if seeds is None else len(seeds), P(mse), P(tgtu), P(pred) if E > 1 else None, None)
    assert rc == expect, (rc, c.lib.dd_last_error(c.handle))
    pick = lambda buf, rows: buf[:(k + 1) * rows * B_all].reshape(k + 1, rows, B_all)[k, :, b0:b0 + B].copy()
    return dict(mse=pick(mse, E), tgtu=pick(tgtu, E), pred=pick(pred, E - 1) if E > 1 else np.zeros((0, B), F32), whole=(mse, tgtu, pred), args=a)


def written_mask(E_rows, B, b0, B_all, k, size):
    """True at the elements of a whole result buffer the launch may write: rows k E_rows .. + E_rows - 1, columns b0 .. b0 + B - 1"""
    m = np.zeros(size, bool)
    body = m[:(k + 1) * E_rows * B_all].reshape(k + 1, E_rows, B_all)
    body[k, :, b0:b0 + B] = True
    return m


def tgtu_ref(x0, m, z, ka, kb, row, mutant=None):
    """(tgtu64 [B], bound [B], d [B, C, S, S]) of one exit plane m from the fp32 operands, x_t in fp32 as the kernel forms it, then float64.
    The bound (u = 2^-24): d = fl(m - tgt) is off by dd = u |d| + dt with dt = 3 u (|tz z| + |t0 x0| + |tx x_t|) as error_ref;
    tanh is 1-Lipschitz, so scan_tanh_abs(d) is off by at most E_TANH + dd; the sum of the non-negative terms passes through at most
    D = C ceil(S S / 256) + 6 + 3 additions and one division:  |tgtu - tgtu64| <= ((D + 4) u sum tanh|d_i| + sum (E_TANH + dd_i)) / (C S S).
    mutant: a wrong reference the tests must tell from the kernel -- "square" (d^2 for tanh|d|), "signed" (tanh d), "last_pixel" (the last
    pixel's channels left out)."""
    B, Cn, S, _ = x0.shape
    xt = (F32(ka) * x0 + F32(kb) * z).astype(np.float64)
    tz, t0, tx = (float(F32(v)) for v in row)
    z64, x64 = z.astype(np.float64), x0.astype(np.float64)
    tgt = tz * z64 + t0 * x64 + tx * xt
    dt = 3 * U24 * (np.abs(tz * z64) + np.abs(t0 * x64) + np.abs(tx * xt))
    d = m.astype(np.float64) - tgt
    term = {None: np.tanh(np.abs(d)), "square": d * d, "signed": np.tanh(d), "last_pixel": np.tanh(np.abs(d))}[mutant].copy()
    if mutant == "last_pixel":
        term[:, :, -1, -1] = 0.0
    n = Cn * S * S
    depth = Cn * -(-S * S // 256) + 6 + 3
    dd = U24 * np.abs(d) + dt
    bound = ((depth + 4) * U24 * np.tanh(np.abs(d)).sum((1, 2, 3)) + (E_TANH + dd).sum((1, 2, 3))) / n
    return term.sum((1, 2, 3)) / n, bound, d


def _images(B, mp, seed):
    g = torch.Generator().manual_seed(seed)
    x0 = (torch.rand(B, mp.in_chans, mp.img_size, mp.img_size, generator=g) * 2 - 1).cuda().contiguous()
    y = torch.randint(0, mp.num_classes, (B,), generator=g).cuda() if mp.num_classes > 0 else None
    return x0, y


def _scan(loop, em, x0, rows, y=None, stream=None, **kw):
    """loop: engine.scan_error_loop (-> err as numpy) or engine.scan_exits_loop (-> its three tables as numpy), on a side stream"""
    stream = side_stream() if stream is None else stream
    with torch.cuda.stream(stream):
        out = loop(em.ctx, em, x0, rows, y=y, stream=stream, **kw)
    stream.synchronize()
    return out.cpu().numpy() if torch.is_tensor(out) else tuple(o.cpu().numpy() for o in out)
