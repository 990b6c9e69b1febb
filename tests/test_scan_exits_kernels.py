"""scan_exits_error_kernel (csrc/scan.hip) alone, through dd_dev_scan_exits_error (GPU).

The old kernel is the reference for order and arithmetic: mse[l] must be bit-equal to dd_dev_scan_error on plane l.  Both sums against
float64 of the same fp32 operands (mse under scan_support.error_ref's bound, tgtu under scan_support.tgtu_ref's); scan_tanh_abs
on the device against its numpy mirror, bit for bit; one element of one plane moved by 1; wrong references the gate must refuse; the copy
of the probes' predictions, the canaries, the fences; the step state's hand-off to row `next`; seeded images; the launcher's refusals."""
import ctypes as C

import numpy as np
import pytest

import kernel_support as ks
from duodiff_amd import _lib
from duodiff_amd.threshold_scan import tanh_abs_f32
from kernel_support import F32, P, untouched
from scan_support import E_TANH, KA, KB, ROWS, SEED, _seeds, draw, error, error_ref, exits_args, exits_error, tgtu_ref, written_mask

pytestmark = pytest.mark.gpu


# (B, C, S, exits): a mostly idle workgroup and one exit; four exits; two exits of one channel; two channels and a second pass that 33
# threads take; every thread looping and the largest shipped depth + 1
SHAPES = [(1, 3, 6, 1), (3, 4, 8, 4), (5, 1, 16, 2), (2, 2, 17, 3), (2, 3, 64, 22)]


def _geometry(B):
    return dict(b0=2, B_all=B + 5)


def _inputs(B, Cn, S, E, seed, hi=3.0):
    """x0, the E planes (standard normal times a scale that rises from 0.3 at the first exit to `hi` at the last) and the predictions"""
    r = np.random.default_rng(seed)
    x0 = r.uniform(-1.0, 1.0, (B, Cn, S, S)).astype(F32)
    planes = (r.standard_normal((E, B, Cn, S, S)) * np.linspace(0.3, hi, E)[:, None, None, None, None]).astype(F32)
    cls = r.uniform(-0.2, 1.0, (max(E - 1, 0), B)).astype(F32)
    return x0, planes, cls


@pytest.mark.parametrize("seeded", [False, True], ids=["plain", "seeded"])
@pytest.mark.parametrize("par", ["predict_noise", "predict_original"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-C%d-S%d-E%d" % s)
def test_exits_bit_equal_with_the_old_kernel_and_against_float64(shape, par, seeded):
    B, Cn, S, E = shape
    g = _geometry(B)
    seeds = _seeds(g["B_all"]) if seeded else None
    x0, planes, cls = _inputs(B, Cn, S, E, 21)
    z = draw(B, Cn, S, ctr=4, seeds=seeds, **g)
    r = exits_error(x0, planes, cls, row=ROWS[par], ka=KA, kb=KB, ctr=4, k=3, seeds=seeds, seed=SEED, **g)
    worst_m = worst_u = 0.0
    for l in range(E):
        old = error(x0, planes[l], row=ROWS[par], ctr=4, seeds=seeds, **g)[0]
        assert np.array_equal(old.view(np.uint32), r["mse"][l].view(np.uint32)), f"mse of exit {l} is not bit-equal to scan_error_kernel on its plane"
        want, bound, _ = error_ref(x0, planes[l], z, KA, KB, ROWS[par])
        worst_m = max(worst_m, ks.gate(r["mse"][l], want, bound, f"mse exit {l} {par}"))
        wantu, boundu, _ = tgtu_ref(x0, planes[l], z, KA, KB, ROWS[par])
        worst_u = max(worst_u, ks.gate(r["tgtu"][l], wantu, boundu, f"tgtu exit {l} {par}"))
        assert (wantu > 0.05).all() and (wantu < 1).all()
    print(f"{(B, Cn, S, E)} {par} {'seeded' if seeded else 'plain'}: mse observed / bound {worst_m:.3f}  tgtu observed / bound {worst_u:.3f}")
    # the copy of the predictions, bit for bit; nothing outside the contract written; the fences (NaN) not read
    assert np.array_equal(r["pred"].view(np.uint32), cls.view(np.uint32))
    for buf, rows in zip(r["whole"], (E, E, E - 1)):
        if rows:
            mask = written_mask(rows, B, g["b0"], g["B_all"], 3, buf.size)
            assert untouched(buf[~mask]), "a byte outside the contract lost its canary"
            assert np.isfinite(buf[mask]).all()
    a = r["args"]
    assert (a.t_out, a.t_final_out, a.t_model_out) == (500, 500, 500.0)


def test_scan_tanh_abs_on_the_device_is_the_numpy_mirror_bit_for_bit():
    """C = 1, S = 1, one exit, the row (0, 0, 0): tgt = 0, d = m, and tgtu = (0 + tanh|d|) / 1 is the function value itself"""
    B = 4096
    r = np.random.default_rng(5)
    d = np.concatenate([np.linspace(0.0, 12.0, 3000), r.uniform(0, 10, 1000), [0.0, 1e-45, 1e-38, 1e-20, 9.999999, 10.0, 10.000001, 11.0, 1e30, np.inf],
                        -r.uniform(0, 12, 86)]).astype(F32)
    assert d.size == B
    out = exits_error(np.zeros((B, 1, 1, 1), F32), d.reshape(1, B, 1, 1, 1), None, 0, B, (0.0, 0.0, 0.0), KA, KB, k=0, ctr=0, seed=SEED)
    got = out["tgtu"][0]
    want = tanh_abs_f32(d)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{int((got != want).sum())} of {B} values differ from the mirror"
    assert got[d == 0].max() == 0 and got.min() >= 0 and got.max() <= 1
    fin = np.isfinite(d)
    err = np.abs(got[fin].astype(np.float64) - np.tanh(np.abs(d[fin].astype(np.float64)))).max()
    print(f"device scan_tanh_abs: max error against float64 tanh {err:.3e} (E_TANH {E_TANH:.3e})")
    assert err <= E_TANH
    with np.errstate(over="ignore"):
        assert np.array_equal(out["mse"][0], (d * d).astype(F32))


@pytest.mark.parametrize("shape", [(3, 4, 8, 4), (2, 3, 64, 2)], ids=lambda s: "B%d-C%d-S%d-E%d" % s)
def test_one_element_moved_by_one_and_mutant_references(shape):
    B, Cn, S, E = shape
    g = _geometry(B)
    par = "predict_noise"
    x0, planes, cls = _inputs(B, Cn, S, E, 33, hi=1.0)       # (the bound grows with the error itself: unit-size residuals keep a move of 1 / n clear of it)
    z = draw(B, Cn, S, ctr=6, **g)
    run = lambda pl: exits_error(x0, pl, cls, row=ROWS[par], ka=KA, kb=KB, ctr=6, seed=SEED, **g)
    n = Cn * S * S
    # the first, the last, one past the 256-thread stride (where the image has one), the middle.  Each of these elements is first put 0.1
    # beside its target (predict_noise: z), where tanh is steep: a move of 1 away from the target then moves the tanh sum by
    # (tanh 1.1 - tanh 0.1) / n = 0.70 / n, clear of the bound at every shape, so both assertions always fire
    cases = ((0, 0, 0), (E - 1, B - 1, n - 1), (E // 2, 0, min(256, n - 2)), (E - 1, B - 1, n // 2))
    for l, b, e in cases:
        planes[l].reshape(B, n)[b, e] = z.reshape(B, n)[b, e] + F32(0.1)
    base = run(planes)
    for l, b, e in cases:
        want, bound, d = error_ref(x0, planes[l], z, KA, KB, ROWS[par])
        wantu, boundu, _ = tgtu_ref(x0, planes[l], z, KA, KB, ROWS[par])
        assert 0.05 < d.reshape(B, n)[b, e] < 0.15
        p2 = planes.copy()
        p2[l].reshape(B, n)[b, e] += F32(1.0)
        got2 = run(p2)
        want2, bound2, _ = error_ref(x0, p2[l], z, KA, KB, ROWS[par])
        wantu2, boundu2, _ = tgtu_ref(x0, p2[l], z, KA, KB, ROWS[par])
        moved, movedu = (want2 - want)[b], (wantu2 - wantu)[b]
        assert moved >= 0.99 / n and moved > 3 * (bound[b] + bound2[b]), "the moved element is below the resolution of the mse test"
        assert abs((float(got2["mse"][l, b]) - float(base["mse"][l, b])) - moved) <= bound[b] + bound2[b], f"element {e} of exit {l} is not in the mse sum"
        assert movedu >= 0.69 / n and movedu > 3 * (boundu[b] + boundu2[b]), "the moved element is below the resolution of the tanh test"
        assert abs((float(got2["tgtu"][l, b]) - float(base["tgtu"][l, b])) - movedu) <= boundu[b] + boundu2[b], f"element {e} of exit {l} is not in the tanh sum"
        keep = np.ones((E, B), bool)
        keep[l, b] = False
        for name in ("mse", "tgtu"):
            assert np.array_equal(got2[name][keep].view(np.uint32), base[name][keep].view(np.uint32)), f"{name}: another exit or image moved"
        assert np.array_equal(got2["pred"], base["pred"])
    # wrong references must fail the gate that the kernel passes
    l = E - 1
    wantu, boundu, _ = tgtu_ref(x0, planes[l], z, KA, KB, ROWS[par])
    ks.gate(base["tgtu"][l], wantu, boundu, "tgtu")
    for mutant in ("square", "signed", "last_pixel"):
        with pytest.raises(AssertionError):
            ks.gate(base["tgtu"][l], tgtu_ref(x0, planes[l], z, KA, KB, ROWS[par], mutant)[0], boundu, mutant)
    with pytest.raises(AssertionError):          # the last exit skipped: the plane before it in its place
        ks.gate(base["tgtu"][l], tgtu_ref(x0, planes[l - 1], z, KA, KB, ROWS[par])[0], boundu, "last exit skipped")
    with pytest.raises(AssertionError):
        ks.gate(base["mse"][l], error_ref(x0, planes[l - 1], z, KA, KB, ROWS[par])[0], error_ref(x0, planes[l], z, KA, KB, ROWS[par])[1], "last exit skipped")
    _, bound, d = error_ref(x0, planes[l], z, KA, KB, ROWS[par])
    sq = d * d
    sq[:, :, -1, -1] = 0.0                       # the last pixel skipped in the mse sum
    with pytest.raises(AssertionError):
        ks.gate(base["mse"][l], sq.sum((1, 2, 3)) / n, bound, "last pixel skipped")


def test_state_advances_only_when_asked_to_row_next():
    B, Cn, S, E = 3, 3, 8, 3
    x0, planes, cls = _inputs(B, Cn, S, E, 41)
    kw = dict(row=ROWS["predict_noise"], ka=KA, kb=KB, k=5, t=731, nxt=17, ctr=9, seed=SEED)
    base = exits_error(x0, planes, cls, 1, 6, advance=0, **kw)
    a0 = base["args"]
    assert (a0.t_out, a0.t_final_out, a0.t_model_out) == (731, 731, 500.0)
    adv = exits_error(x0, planes, cls, 1, 6, advance=1, **kw)
    a1 = adv["args"]
    assert (a1.t_out, a1.t_final_out, a1.t_model_out) == (17, 731, 250.0)        # row `next` and its t_model; t_final stays
    for name in ("mse", "tgtu", "pred"):
        assert np.array_equal(base[name], adv[name])
    # the output row is ctr - counter_base whatever the timestep: another k with the same ctr - k base, the same numbers
    other = exits_error(x0, planes, cls, 1, 6, advance=0, **{**kw, "k": 0, "t": 3, "nxt": 999})
    for name in ("mse", "tgtu", "pred"):
        assert np.array_equal(base[name], other[name])


@pytest.mark.parametrize("shape", [(3, 4, 8, 4), (5, 1, 16, 2)], ids=lambda s: "B%d-C%d-S%d-E%d" % s)
def test_a_seeded_image_does_not_depend_on_its_batch(shape):
    B, Cn, S, E = shape
    g = _geometry(B)
    seeds = _seeds(g["B_all"] + 3)
    x0, planes, cls = _inputs(B, Cn, S, E, 51)
    kw = dict(row=ROWS["predict_noise"], ka=KA, kb=KB, ctr=12, seed=SEED)
    got = exits_error(x0, planes, cls, seeds=seeds, **g, **kw)
    for b in (0, B - 1):
        alone = exits_error(x0[b:b + 1], planes[:, b:b + 1], cls[:, b:b + 1], 0, 1, seeds=seeds[g["b0"] + b:g["b0"] + b + 1], **kw)
        for name in ("mse", "tgtu", "pred"):
            assert np.array_equal(alone[name][:, 0], got[name][:, b]), f"{name}: image {b} alone differs from the image in its batch"
    moved = exits_error(x0, planes, cls, 5, g["B_all"] + 3, seeds=np.roll(seeds, 3), **{**kw, "k": 1})
    assert np.array_equal(moved["mse"], got["mse"]) and np.array_equal(moved["tgtu"], got["tgtu"])
    assert not np.array_equal(exits_error(x0, planes, cls, seeds=seeds, **g, **{**kw, "ctr": 14})["mse"], got["mse"])      # another counter: another z


def test_the_launcher_refuses_before_any_launch():
    """What the dev entry refuses, with nothing launched.  As with dd_dev_scan_error, the entry checks C, the exit count and the null pointers
    itself before it calls launch_scan_exits_error, so the launcher's own guards (exits outside 1..32, B_all < b0 + B, null pointers) are a
    second line that this test does not reach; the loop's refusal of depth + 1 > 32 is in test_scan_exits_loop.py."""
    c = ks.ctx()
    x = np.zeros((1, 1, 4, 4), F32)
    many = np.zeros((40, 1, 1, 4, 4), F32)
    cases = ((dict(Cn=5), _lib.DD_ERR_UNSUPPORTED), (dict(Cn=2, S=4096), _lib.DD_ERR_UNSUPPORTED), (dict(exits=33), _lib.DD_ERR_UNSUPPORTED),
             (dict(exits=0), _lib.DD_ERR_INVALID), (dict(Cn=0), _lib.DD_ERR_INVALID), (dict(b0=3, B_all=3), _lib.DD_ERR_INVALID),
             (dict(k=-1), _lib.DD_ERR_INVALID), (dict(B=0), _lib.DD_ERR_INVALID), (dict(t=1000), _lib.DD_ERR_INVALID),
             (dict(nxt=-1), _lib.DD_ERR_INVALID), (dict(k=2, ctr=1), _lib.DD_ERR_INVALID))
    for kw, status in cases:
        p = dict(B=1, Cn=1, S=4, exits=2, b0=0, B_all=1, k=0, t=5, nxt=4, ctr=0)
        p.update(kw)
        a = exits_args(p["B"], p["Cn"], p["S"], p["exits"], p["b0"], p["B_all"], p["k"], p["t"], p["nxt"], KA, KB, (1.0, 0.0, 0.0), p["ctr"])
        outs = [np.zeros(4096, F32) for _ in range(3)]
        rc = c.lib.dd_dev_scan_exits_error(c.handle, C.byref(a), P(x), P(many), P(x), P(x), None, 0, P(outs[0]), P(outs[1]), P(outs[2]), None)
        assert rc == status, (kw, rc)
        assert not any(o.any() for o in outs) and a.t_out == -12345
    a = exits_args(1, 1, 4, 2, 0, 1, 0, 5, 4, KA, KB, (1.0, 0.0, 0.0), 0)
    o = np.zeros(64, F32)
    assert c.lib.dd_dev_scan_exits_error(c.handle, C.byref(a), P(x), None, P(x), P(x), None, 0, P(o), P(o), P(o), None) == _lib.DD_ERR_INVALID    # two exits, no outs
    assert c.lib.dd_dev_scan_exits_error(c.handle, C.byref(a), P(x), P(x), P(x), P(x), P(_seeds(1)), 0, P(o), P(o), P(o), None) == _lib.DD_ERR_INVALID
    assert not o.any()
