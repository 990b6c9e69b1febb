"""The two kernels of the denoising-error scan (csrc/scan.hip) alone, through dd_dev_scan_diffuse / dd_dev_scan_error (GPU).

diffuse: the draw (its own Philox stream word, the site of draw_site with and without per-image seeds), x_t bit for bit against numpy float32
in step_update.h's order, the canaries around the output.
error: against float64 of the same fp32 operands under a derived bound, for the three target rows; one element of m moved by 1; an image alone,
in a batch and at another b0; the advance of the step state.

The bound of the error kernel (u = 2^-24).  Per element the kernel forms tgt = fl(fl(fl(tz z) + fl(t0 x0)) + fl(tx x_t)): three products and two
sums, each rounding at most u times a partial sum that A = |tz z| + |t0 x0| + |tx x_t| bounds, so |tgt - tgt64| <= 3 u A =: dt.  d = fl(m - tgt)
is off by dt + u |d|, its square d^2 by 2 |d| (dt + u |d|) + u d^2 = 3 u d^2 + 2 |d| dt.  The kernel states its summation depth: no term passes
through more than D = C ceil(S S / 256) + 6 + 3 additions, each rounding at most u of a sum of non-negative terms, then one division:
    |err - err64| <= ((D + 4) u sum d_i^2 + sum 2 |d_i| dt_i) / (C S S)
with d_i, dt_i from the float64 restatement."""
import ctypes as C
import math

import numpy as np
import pytest

import kernel_support as ks
from duodiff_amd import _lib
from kernel_support import F32, P, untouched
from scan_support import KA, KB, ROWS, SEED, _args, _seeds, diffuse, draw, error, error_ref, z_ref
from test_final_step import PHILOX_BOUND

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3, 6), (3, 4, 8), (5, 1, 16), (2, 2, 17), (2, 3, 64)]       # (B, C, S): most of a workgroup idle .. every thread loops


def _geometry(B):
    """every case: the launch starts at image b0 > 0 of a whole batch B_all > B"""
    return dict(b0=2, B_all=B + 5)


def _inputs(B, Cn, S, seed):
    r = np.random.default_rng(seed)
    return r.uniform(-1.0, 1.0, (B, Cn, S, S)).astype(F32), r.standard_normal((B, Cn, S, S)).astype(F32)


# ---------------------------------------------------------------------------------------------------------------- diffuse
@pytest.mark.parametrize("seeded", [False, True], ids=["plain", "seeded"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-C%d-S%d" % s)
def test_diffuse_the_draw(shape, seeded):
    B, Cn, S = shape
    g = _geometry(B)
    seeds = _seeds(g["B_all"]) if seeded else None
    z = draw(B, Cn, S, ctr=17, seeds=seeds, **g).astype(np.float64)
    n = z.size
    mean, var = z.mean(), z.var()
    print(f"{shape} {'seeded' if seeded else 'plain'}: n {n} mean {mean:+.4f} (bound {5 / math.sqrt(n):.4f}) var {var:.4f} (|var - 1| bound {5 * math.sqrt(2 / n):.4f})")
    assert abs(mean) <= 5 / math.sqrt(n) and abs(var - 1) <= 5 * math.sqrt(2 / n)
    # the site, the counter and the stream word: the host's Philox with the scan's stream word, under the suite's bound on the hardware log / sin / cos
    ratio = ks.gate(z, z_ref(B, Cn, S, g["b0"], 17, seeds, SEED), PHILOX_BOUND, "scan z against philox_normal4_ref")
    print(f"  max |z - ref| / bound {ratio:.3f}")
    # ... and not the sampling step's draw, nor the draw of another counter
    step = (ks.final_philox_ref(SEED, B, Cn, S, g["b0"], 17, ks.PHILOX_STEP)[0] if not seeded
            else np.concatenate([ks.final_philox_ref(int(seeds[g["b0"] + b]), 1, Cn, S, 0, 17, ks.PHILOX_STEP)[0] for b in range(B)]))
    assert np.abs(z - step).max() > 0.5
    assert np.abs(z - draw(B, Cn, S, ctr=18, seeds=seeds, **g)).max() > 0.5


def test_diffuse_z_differs_from_the_sampling_loops_draw_at_the_same_counter():
    """against the z a device loop draws (loop_support.philox_z: PHILOX_STEP) under the same seed, counter and pixel ids"""
    import torch
    from conftest import TINY
    from loop_support import philox_z, side_stream, uvit
    B, Cn, S = 3, 3, 8
    em = uvit(TINY, 3, "bf16", B)[0].engine_model(B)
    zl = philox_z(em, torch.zeros(B, Cn, S, S, device="cuda"), 17, SEED, side_stream()).cpu().numpy()
    zs = draw(B, Cn, S, 0, B, ctr=17)
    assert np.isfinite(zl).all() and np.abs(zl - zs).max() > 0.5
    ks.gate(zl, ks.final_philox_ref(SEED, B, Cn, S, 0, 17, ks.PHILOX_STEP)[0], PHILOX_BOUND, "the loop's z is the PHILOX_STEP draw")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-C%d-S%d" % s)
def test_diffuse_a_seeded_image_does_not_depend_on_its_batch(shape):
    B, Cn, S = shape
    g = _geometry(B)
    seeds = _seeds(g["B_all"])
    z = draw(B, Cn, S, ctr=5, seeds=seeds, **g)
    for b in (0, B - 1):
        alone = draw(1, Cn, S, 0, 1, ctr=5, seeds=seeds[g["b0"] + b:g["b0"] + b + 1])
        assert np.array_equal(alone[0], z[b]), f"image {b} alone differs from the image in its batch"
        plain = draw(1, Cn, S, 0, 1, ctr=5, seed=int(seeds[g["b0"] + b]))       # the plain B = 1 call under that seed
        assert np.array_equal(plain[0], z[b])
    # unseeded, the image's place in the batch is part of the draw
    assert not np.array_equal(draw(B, Cn, S, 0, g["B_all"], ctr=5)[0], draw(B, Cn, S, 1, g["B_all"], ctr=5)[0])
    assert np.array_equal(draw(B + 1, Cn, S, 0, g["B_all"], ctr=5)[1:], draw(B, Cn, S, 1, g["B_all"], ctr=5))


@pytest.mark.parametrize("seeded", [False, True], ids=["plain", "seeded"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-C%d-S%d" % s)
def test_diffuse_general_rows_bit_equal_and_canaries(shape, seeded):
    B, Cn, S = shape
    g = _geometry(B)
    seeds = _seeds(g["B_all"]) if seeded else None
    x0, _ = _inputs(B, Cn, S, 11)
    z = draw(B, Cn, S, ctr=9, seeds=seeds, **g)
    for ka, kb in ((KA, KB), (F32(0.99995), F32(0.01)), (F32(-1.5), F32(2.25)), (F32(0.7), F32(0.0))):
        xt, whole, a = diffuse(x0, ka=ka, kb=kb, ctr=9, seeds=seeds, **g)
        want = F32(ka) * x0 + F32(kb) * z if kb != 0 else F32(ka) * x0          # each product and the sum rounded to fp32 on its own
        assert want.dtype == F32 and np.array_equal(xt, want), f"row ({ka}, {kb}): x_t is not bit-equal to numpy float32"
        assert untouched(whole[:8]) and untouched(whole[8 + x0.size:]), "a canary around the output was written"
        assert (a.t_out, a.t_final_out, a.t_model_out) == (3, 3, 500.0)             # the first kernel of a step leaves the state alone


# ---------------------------------------------------------------------------------------------------------------- error
@pytest.mark.parametrize("seeded", [False, True], ids=["plain", "seeded"])
@pytest.mark.parametrize("par", sorted(ROWS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-C%d-S%d" % s)
def test_error_against_float64(shape, par, seeded):
    B, Cn, S = shape
    g = _geometry(B)
    seeds = _seeds(g["B_all"]) if seeded else None
    x0, m = _inputs(B, Cn, S, 21)
    z = draw(B, Cn, S, ctr=4, seeds=seeds, **g)
    got, whole, a = error(x0, m, row=ROWS[par], ctr=4, seeds=seeds, **g)
    want, bound, d = error_ref(x0, m, z, KA, KB, ROWS[par])
    ratio = ks.gate(got, want, bound, f"err {par}")
    print(f"{shape} {par} {'seeded' if seeded else 'plain'}: err {want.round(4).tolist()} observed / bound {ratio:.3f} (bound / err {float((bound / want).max()):.2e})")
    assert (want > 0.1).all()
    # nothing but the B results was written, and the fences around x0 and m (NaN) did not reach them
    k, lo = 3, 3 * g["B_all"] + g["b0"]
    assert untouched(whole[:lo]) and untouched(whole[lo + B:]) and np.isfinite(got).all()
    assert (a.t_out, a.t_final_out, a.t_model_out) == (k, k, 500.0)
    # one element of m moved by 1 (away from the target) moves the result by (2 |d| + 1) / CHW >= 1 / CHW: the first, the last, one past the
    # 256-thread stride, one in the middle
    n = Cn * S * S
    for b, e in ((0, 0), (B - 1, n - 1), (0, min(256, n - 1)), (B - 1, n // 2)):
        m2 = m.copy()
        m2.reshape(B, n)[b, e] += F32(1.0) if d.reshape(B, n)[b, e] >= 0 else F32(-1.0)
        got2 = error(x0, m2, row=ROWS[par], ctr=4, seeds=seeds, **g)[0]
        want2, bound2, _ = error_ref(x0, m2, z, KA, KB, ROWS[par])
        moved = (want2 - want)[b]
        assert moved >= 0.99 / n and moved > 3 * (bound[b] + bound2[b]), "the moved element is below the resolution of the test"
        assert abs((float(got2[b]) - float(got[b])) - moved) <= bound[b] + bound2[b], f"element {e} of image {b} is not in the sum"
        others = np.arange(B) != b
        assert np.array_equal(got2[others], got[others])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-C%d-S%d" % s)
def test_error_a_seeded_image_does_not_depend_on_its_batch(shape):
    B, Cn, S = shape
    g = _geometry(B)
    seeds = _seeds(g["B_all"] + 3)
    x0, m = _inputs(B, Cn, S, 31)
    row = ROWS["predict_previous"]
    got = error(x0, m, row=row, ctr=2, seeds=seeds, **g)[0]
    for b in (0, B - 1):
        alone = error(x0[b:b + 1], m[b:b + 1], 0, 1, row, ctr=2, seeds=seeds[g["b0"] + b:g["b0"] + b + 1])[0]
        assert alone[0] == got[b], f"image {b} alone differs from the image in its batch"
    moved = error(x0, m, 5, g["B_all"] + 3, row, k=1, ctr=2, seeds=np.roll(seeds, 3))[0]         # another b0, another row, the same seeds per image
    assert np.array_equal(moved, got)
    assert not np.array_equal(error(x0, m, row=row, ctr=3, seeds=seeds, **g)[0], got)             # another counter: another z


def test_error_advance_only_when_asked():
    B, Cn, S = 3, 3, 8
    x0, m = _inputs(B, Cn, S, 41)
    base, _, a0 = error(x0, m, 1, 6, ROWS["predict_noise"], k=5, advance=0)
    assert (a0.t_out, a0.t_final_out, a0.t_model_out) == (5, 5, 500.0)
    adv, _, a1 = error(x0, m, 1, 6, ROWS["predict_noise"], k=5, advance=1)
    assert (a1.t_out, a1.t_final_out, a1.t_model_out) == (6, 5, 250.0)              # t + 1 and the next row's t_model; t_final stays
    assert np.array_equal(base, adv)


def test_launchers_refuse_a_shape_before_any_launch():
    c = ks.ctx()
    x = np.zeros((1, 1, 4, 4), F32)
    for kw, status in ((dict(Cn=5), _lib.DD_ERR_UNSUPPORTED), (dict(Cn=2, S=4096), _lib.DD_ERR_UNSUPPORTED), (dict(Cn=0), _lib.DD_ERR_INVALID),
                       (dict(b0=3, B_all=3), _lib.DD_ERR_INVALID), (dict(k=-1), _lib.DD_ERR_INVALID), (dict(B=0), _lib.DD_ERR_INVALID)):
        p = dict(B=1, Cn=1, S=4, b0=0, B_all=1, k=0)
        p.update(kw)
        for entry in ("diffuse", "error"):
            a = _args(p["B"], p["Cn"], p["S"], p["b0"], p["B_all"], p["k"], KA, KB)
            out = np.zeros(64, F32)
            if entry == "diffuse":
                rc = c.lib.dd_dev_scan_diffuse(c.handle, C.byref(a), P(x), None, 0, P(out), None)
            else:
                rc = c.lib.dd_dev_scan_error(c.handle, C.byref(a), P(x), P(x), None, 0, P(out), None)
            assert rc == status, (entry, kw, rc)
            assert not out.any() and a.t_out == -12345
    a = _args(1, 1, 4, 0, 1, 0, KA, KB)
    out = np.zeros(64, F32)
    assert c.lib.dd_dev_scan_diffuse(c.handle, C.byref(a), P(x), P(_seeds(1)), 0, P(out), None) == _lib.DD_ERR_INVALID      # seeds without a count
    a.b0, a.B_all = 1, 2
    assert c.lib.dd_dev_scan_diffuse(c.handle, C.byref(a), P(x), P(_seeds(1)), 1, P(out), None) == _lib.DD_ERR_INVALID      # fewer seeds than b0 + B
    assert c.lib.dd_dev_scan_error(c.handle, C.byref(a), P(x), None, None, 0, P(out), None) == _lib.DD_ERR_INVALID
