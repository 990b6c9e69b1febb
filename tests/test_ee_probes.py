"""The early-exit probes of csrc/rowops.hip one by one, each through its production launch_* function on host arrays (include/duodiff_dev.h
dd_dev_ee_probe, dd_dev_ee_probe_reduce, dd_dev_ee_attn_probe) against the float64 restatements of tests/kernel_support.py, at the widths the
shipped models have (embed_dim 256 .. 1024, 257 / 258 tokens) and at the sizes where a loop of theirs takes another trip or a slice ends;
tests/test_kernel_support.py proves on the CPU that the inputs used here see each deliberate error of those restatements.  Every output comes
back whole with DD_DEV_EE_TAIL canary elements behind it.

ee_probe_rows_kernel: s = sigmoid(x . w + b) per token row, bound kernel_support.probe_rows_ref (the logit's (D / 64 + 8) roundings through the
sigmoid's slope, expf's 4 ulp, the add and the divide).  ee_probe_reduce_kernel: the mean of the rows, (ceil(L / 64) + 7) u relative, and bit
for bit the float32 emulation of its fixed order.  ee_attn_probe_kernel: kernel_support.attn_probe_ref, from the module's RAW parameters with
bk kept, the bound carried elementwise through scores, softmax, xbar, the two mat-vecs, SiLU and the last dot.

Largest error / bound seen on the MI355X (each test prints its own): rows 0.49, their mean 0.02 against the float64 rows and 0.26 against the
kernel's own rows; the reduce alone 0.28; the attention probe 0.0003 -- its bound is the worst case through (D / 64 + 7) roundings of scores of
magnitude sum |u| |x| and a chain of L - 1 fmas, a few thousand times what the kernel's errors add up to (1e-8 .. 4e-6 here), and every mutant
of kernel_support.attn_probe_ref is 13 bounds away or more (tests/test_kernel_support.py).
"""
import numpy as np
import pytest

import kernel_support as ks
from kernel_support import EE_B, EE_TAIL, P, gate, untouched

gpu = pytest.mark.gpu


def _rows_and_mean(case, srow, out, what):
    """gates the rows against float64, the mean against float64 (with the rows' bound) and against the kernel's own rows; -> the three ratios"""
    B, L = case["B"], case["L"]
    s, tol_s = ks.probe_rows_ref(case["x"], case["w"], case["b"])
    got_s = srow[:B * L].reshape(B, L)
    r_rows = gate(got_s, s, tol_s, f"{what}: rows")
    assert untouched(srow[B * L:]) and untouched(out[B:])
    r_mean = gate(out[:B], *ks.probe_mean_ref(s, tol_s), f"{what}: mean against the float64 rows")
    r_own = gate(out[:B], *ks.probe_mean_ref(got_s), f"{what}: mean against the kernel's own rows")
    return r_rows, r_mean, r_own


@gpu
@pytest.mark.parametrize("D,L", ks.EE_PROBE_CASES)
def test_ee_probe_rows_and_mean_against_float64_reference(D, L):
    """launch_ee_probe with its reduce, and rows only + launch_ee_probe_reduce: the same bits; every row and every mean within its bound.
    MI355X: largest error / bound over all cases, rows 0.49, mean against the float64 rows 0.02, mean against the kernel's own rows 0.26"""
    case = ks.ee_probe_case(EE_B, L, D)
    srow, out = ks.run_ee_probe(case)
    r = _rows_and_mean(case, srow, out, f"ee_probe D {D} L {L}")
    print(f"ee_probe D {D} L {L}: largest error / bound rows {r[0]:.3f}, mean {r[1]:.3f}, mean of own rows {r[2]:.3f}")
    srow2, none = ks.run_ee_probe(case, reduce=False)
    assert none is None and np.array_equal(srow2.view(np.uint32), srow.view(np.uint32))
    out2 = ks.run_ee_reduce(srow2[:EE_B * L].reshape(EE_B, L))
    assert np.array_equal(out2.view(np.uint32), out.view(np.uint32))


@gpu
def test_ee_probe_selects_its_row_from_the_step_state():
    """per-timestep probes: the launch reads row t t_mul + add of the table with t from the step state; every other row is NaN.  A row outside
    the table is refused with nothing written.  MI355X: largest error / bound rows 0.48, mean 0.007"""
    D, L, nl, add = 512, 17, 4, 2
    for t in (0, 3, 6):
        case = ks.ee_probe_case(EE_B, L, D, n_probe=7 * nl, row=t * nl + add)
        srow, out = ks.run_ee_probe(case, t_state=t, t_mul=nl, add=add)
        r = _rows_and_mean(case, srow, out, f"ee_probe row {t} * {nl} + {add}")
        print(f"ee_probe t {t}: largest error / bound rows {r[0]:.3f}, mean {r[1]:.3f}")
    c = ks.ctx()
    srow, out = np.full(EE_B * L + EE_TAIL, 7.0, np.float32), np.full(EE_B + EE_TAIL, 7.0, np.float32)
    for t, t_mul, a in ((7, nl, 0), (6, nl, 4), (0, 0, 28), (6, nl, -1), (-1, nl, 2)):
        with pytest.raises(ValueError):
            c.check(c.lib.dd_dev_ee_probe(c.handle, EE_B, L, D, 7 * nl, t, t_mul, a, P(case["x"]), P(case["pw"]), P(case["pb"]), P(srow), P(out), None))
    assert (srow == 7.0).all() and (out == 7.0).all()


@gpu
@pytest.mark.parametrize("L", ks.EE_REDUCE_L)
@pytest.mark.parametrize("rows", ks.EE_REDUCE_ROWS)
def test_ee_probe_reduce(rows, L):
    """launch_ee_probe_reduce alone (rows: one wave per row, four per workgroup): within the float64 bound, and the bits of the float32
    emulation of its fixed order.  MI355X: largest error / bound 0.28"""
    s = ks.ee_reduce_rows(rows, L)
    out = ks.run_ee_reduce(s)
    r = gate(out[:rows], *ks.probe_mean_ref(s), "ee_probe_reduce")
    print(f"ee_probe_reduce rows {rows} L {L}: largest error / bound {r:.3f}")
    assert untouched(out[rows:])
    assert np.array_equal(out[:rows].view(np.uint32), ks.probe_mean_f32(s).view(np.uint32))


@gpu
@pytest.mark.parametrize("D,L", ks.EE_ATTN_CASES)
def test_ee_attn_probe_against_float64_reference(D, L):
    """launch_ee_attn_probe on the operands the model's fold makes of the raw parameters, against the module in float64 with bk kept.
    MI355X: largest error / bound 0.0003 (errors 6e-9 .. 4e-6 against bounds 2e-4 .. 0.4, the larger of each in image 2, whose scores lie near 1e3)"""
    case = ks.ee_attn_case(EE_B, L, D)
    out = ks.run_ee_attn(case)
    want, tol = ks.attn_probe_ref(*(case[k] for k in ("x", "q", "wkv", "bkv", "w0", "b0", "w2", "b2")))
    r = gate(out[:EE_B], want, tol, f"ee_attn_probe D {D} L {L}")
    print(f"ee_attn_probe D {D} L {L}: largest error / bound {r:.5f} (errors {np.abs(out[:EE_B] - want)}, bounds {tol})")
    assert untouched(out[EE_B:])


@gpu
def test_ee_attn_probe_refuses():
    c = ks.ctx()
    case = ks.ee_attn_case(1, 2, 64)
    out = np.full(1 + EE_TAIL, 7.0, np.float32)
    ops = [P(case[k]) for k in ("q", "wkv", "bkv", "w0", "b0", "w2", "b2")]
    for L, D in ((1, 64), (2, 96), (2, 32)):
        with pytest.raises(ValueError):
            c.check(c.lib.dd_dev_ee_attn_probe(c.handle, 1, L, D, P(case["x"]), *ops, P(out), None))
    assert (out == 7.0).all()


@gpu
def test_a_probe_does_not_depend_on_its_batch():
    """image b of a batch of 5 gives the bits of its own call, for both probes (one workgroup row per image, fixed-order reductions)"""
    B, L, D = 5, 258, 512
    case = ks.ee_probe_case(B, L, D)
    srow, out = ks.run_ee_probe(case)
    for b in range(B):
        one = dict(case, B=1, x=np.ascontiguousarray(case["x"][b:b + 1]))
        s1, o1 = ks.run_ee_probe(one)
        assert np.array_equal(s1[:L].view(np.uint32), srow[b * L:(b + 1) * L].view(np.uint32)) and o1[0].view(np.uint32) == out[b].view(np.uint32), b
    acase = ks.ee_attn_case(B, L, D)
    whole = ks.run_ee_attn(acase)
    for b in range(B):
        alone = ks.run_ee_attn(acase, images=slice(b, b + 1))
        assert alone[0].view(np.uint32) == whole[b].view(np.uint32), b


def test_gates_reject_the_bugs_they_are_meant_to_catch():
    """The gates above, fed what a wrong kernel would return on the inputs of one case each: every mutant of kernel_support's restatements
    raises; what a correct kernel returns -- the float32 restatement -- passes."""
    D, L = 512, 257
    case = ks.ee_probe_case(EE_B, L, D)
    s, tol_s = ks.probe_rows_ref(case["x"], case["w"], case["b"])
    mean, tol = ks.probe_mean_ref(s, tol_s)
    s32 = ks.probe_rows_f32(case["x"], case["w"], case["b"])
    assert gate(s32, s, tol_s, "float32 rows") <= 1.0 and gate(ks.probe_mean_f32(s32), mean, tol, "float32 mean") <= 1.0
    for mut in ks.EE_ROW_MUTANTS:
        bad = ks.probe_rows_ref(case["x"], case["w"], case["b"], mutant=mut)[0]
        with pytest.raises(AssertionError):
            gate(bad, s, tol_s, mut)
        with pytest.raises(AssertionError):
            gate(bad.mean(-1), mean, tol, mut + ", in the mean")
    tab = ks.ee_probe_case(EE_B, 17, D, n_probe=28, row=14)
    st, tt = ks.probe_rows_ref(tab["x"], tab["pw"], tab["pb"], row=14)
    with pytest.raises(AssertionError):
        gate(ks.probe_rows_ref(tab["x"], tab["pw"], tab["pb"], row=14, mutant="wrong_probe_row", wrong_row=2)[0], st, tt, "wrong_probe_row")
    own = ks.probe_mean_ref(s32)
    for mut in ks.EE_MEAN_MUTANTS:
        with pytest.raises(AssertionError):
            gate(ks.probe_mean_ref(s32, mutant=mut)[0], *own, mut)
    D, L = 512, 258
    acase = ks.ee_attn_case(EE_B, L, D)
    ops = [acase[k] for k in ("x", "q", "wkv", "bkv", "w0", "b0", "w2", "b2")]
    want, atol = ks.attn_probe_ref(*ops)
    assert gate(ks.attn_probe_f32(*ops), want, atol, "float32 evaluation of the folded form") <= 1.0
    for mut in ks.EE_ATTN_MUTANTS:
        with pytest.raises(AssertionError):
            gate(ks.attn_probe_ref(*ops, mutant=mut)[0], want, atol, mut)
