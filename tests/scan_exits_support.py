"""Shared by the early-exit scan's tests (test_threshold_scan_cpu.py, test_scan_exits_kernels.py, test_scan_exits_loop.py): the measured
constant of scan_tanh_abs, the dev-entry caller of scan_exits_error_kernel and its float64 references.  No GPU at import."""
import ctypes as C

import numpy as np

from kernel_support import F32, U24, P

# The largest |scan_tanh_abs(d) - tanh|d|| over every fp32 d against float64 tanh: tools/scan_tanh_sweep.py (all 1 092 616 193 values of
# [0, 10], the tail, inf), a CPU measurement of the numpy mirror duodiff_amd.threshold_scan.tanh_abs_f32.  The spec is <= 1e-6.
E_TANH = 1.66e-7                        # measured 1.6533e-7, at d = 1.1165210
TANH_BREAKPOINTS = (0.0, 10.0)          # the function's only breakpoints: |d| = 0 (the fabs) and the clamp


def exits_args(B, Cn, S, exits, b0, B_all, k, t, nxt, ka, kb, row, ctr, t_model=500.0, next_t_model=250.0, seed=0, advance=0):
    from duodiff_amd import _lib
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
    import kernel_support as ks
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
    The bound (u = 2^-24): d = fl(m - tgt) is off by dd = u |d| + dt with dt = 3 u (|tz z| + |t0 x0| + |tx x_t|) as test_scan_kernels.error_ref;
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
