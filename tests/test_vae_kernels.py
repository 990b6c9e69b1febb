"""The kernels of csrc/vae_kernels.hip one by one, each through its production launch_* function on host arrays
(dd_dev_vae_gather kinds 2 / 3, dd_dev_groupnorm, dd_dev_softmax_rows, dd_dev_vae_input / _output / _moments, dd_dev_cast) against the
restatements of tests/kernel_support.py; tests/test_kernel_support.py proves on the CPU that the inputs used here see each deliberate error
of those restatements.  Every output comes back whole with DD_DEV_VAE_TAIL canary elements behind it.

Gathers, cast, the NHWC -> NCHW copy: bit for bit.  post_quant_conv and quant_conv: an fmaf chain of n terms started on the bias, bound
(n + 3) 2^-24 (|b| + sum |w| |v|) (+ one rounding for z inv_scale); the sample z: the bound of tests/test_vae_encode.py plus the moments'
errors carried through the sample (kernel_support.vae_moments_ref).  Softmax: kernel_support.softmax_ref.  GroupNorm: against torch's
float64 group_norm (+ silu), |err| <= 8 e32 (+ one bf16 ulp), e32 = the error of torch's own fp32 group_norm on the CPU against float64 on
the elements of that case with the same per-group (mean, std) -- never above the e32 of the whole case.

Largest error / bound seen on the MI355X (each test prints its own): vae_input 0.27; vae_moments 0.17 (moments), 0.12 (z); softmax 0.15
(fp32), 0.50 (bf16: half an ulp of the one granted); GroupNorm 0.35 (fp32), 0.50 (bf16).  GroupNorm's largest err / e32 per (mean, std) pair,
fp32: 2.81, 0.83, 0.56, 0.65 of the 8 allowed; the one-pass statistics that the kernels held before (sums of x and x^2 in fp32) gave
1.58, 29.0, 410 and 1567 on the same inputs and failed every case.
"""
import numpy as np
import pytest

import kernel_support as ks
from kernel_support import P, VAE_TAIL, bf16_bits, gate, untouched, values

pytestmark = pytest.mark.gpu
PRECS = ["bf16", "fp32"]
UNSUPPORTED = NotImplementedError


def _bits(a, prec):
    return bf16_bits(a) if prec == "bf16" else np.ascontiguousarray(a, np.float32)


# ---------------------------------------------------------------- gathers
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("C", ks.GATHER_C)
@pytest.mark.parametrize("kind,B,H,W", ks.GATHER_SHAPES)
def test_im2col3x3_bitwise(kind, B, H, W, C, prec):
    """launch_im2col3x3 plain (kind 2) and through the nearest-2x upsample (kind 3): every element, the zero columns, the canary"""
    src = ks.gather_input(kind, B, H, W, C)
    got, kpad = ks.vae_gather(kind, prec, B, H, W, C, src)
    want = ks.im2col3x3_ref(src, kind == 3, kpad)
    rows = B * H * W
    assert np.array_equal(got[:rows], _bits(want, prec))
    assert (got[:rows, 9 * C:] == 0).all() and untouched(got[rows:])


@pytest.mark.parametrize("prec", PRECS)
def test_input_gather_non_square(prec):
    """the encoder's input path (launch_vae_image + launch_im2col3x3_c4) at H != W"""
    B, H, W = 2, 3, 5
    src = np.random.default_rng(35).integers(-64, 64, (B, 3, H, W)).astype(np.float32) / 64.0
    got, kpad = ks.vae_gather(1, prec, B, H, W, 0, src)
    nhwc = np.zeros((B, H, W, 4), np.float32)
    nhwc[..., :3] = src.transpose(0, 2, 3, 1)
    rows = B * H * W
    assert np.array_equal(got[:rows], _bits(ks.im2col3x3_ref(nhwc, False, kpad), prec)) and untouched(got[rows:])


def test_gather_refuses_what_the_launcher_refuses():
    c = ks.ctx()
    src, dst = np.zeros(2 * 2 * 4, np.uint16), np.zeros(4 * 64 + 64, np.uint16)
    for kind in (2, 3):
        with pytest.raises(UNSUPPORTED, match="16-byte"):      # C = 4 in bf16: half a vector
            c.check(c.lib.dd_dev_vae_gather(c.handle, kind, ks.PREC_BF16, 1, 2, 2, 4, P(src), P(dst), dst.nbytes, None))
    with pytest.raises(ValueError):                              # an odd size cannot be a 2x upsample
        c.check(c.lib.dd_dev_vae_gather(c.handle, 3, ks.PREC_BF16, 1, 3, 2, 8, P(src), P(dst), dst.nbytes, None))


# ---------------------------------------------------------------- cast, vae_output
@pytest.mark.parametrize("prec", PRECS)
def test_cast_bitwise(prec):
    x = ks.cast_inputs()
    c = ks.ctx()
    code, dt = ks._prec(prec)
    out = np.zeros(x.size + VAE_TAIL, dt)
    c.check(c.lib.dd_dev_cast(c.handle, code, x.size, P(x), P(out), None))
    want = bf16_bits(x) if prec == "bf16" else x.view(np.uint32)
    assert np.array_equal(out[:x.size].view(want.dtype), want) and untouched(out[x.size:])


@pytest.mark.parametrize("B,C,HW,ldc", [(3, 3, 35, 4), (2, 3, 300, 4), (2, 8, 9, 8)])
def test_vae_output_bitwise(B, C, HW, ldc):
    inp = np.random.default_rng(HW).standard_normal((B * HW, ldc)).astype(np.float32)
    c = ks.ctx()
    out = np.zeros(B * C * HW + VAE_TAIL, np.float32)
    c.check(c.lib.dd_dev_vae_output(c.handle, B, C, HW, ldc, P(inp), P(out), None))
    want = ks.vae_output_ref(inp, B, C, HW, ldc)
    assert np.array_equal(out[:want.size].view(np.uint32), want.reshape(-1).view(np.uint32)) and untouched(out[want.size:])


# ---------------------------------------------------------------- the 1x1 convolutions
@pytest.mark.parametrize("B,HW", ks.VAE_INPUT_SHAPES)
def test_vae_input(B, HW):
    """post_quant_conv(z / scale) -> NHWC rows.  MI355X: largest error / bound 0.27"""
    a = ks.vae_input_case(B, HW)
    c = ks.ctx()
    out = np.zeros(B * HW * 4 + VAE_TAIL, np.float32)
    c.check(c.lib.dd_dev_vae_input(c.handle, B, HW, P(a["z"]), P(a["w"]), P(a["b"]), float(a["inv_scale"]), P(out), None))
    want, tol = ks.vae_input_ref(a["z"], a["w"], a["b"], a["inv_scale"])
    r = gate(out[:want.size].reshape(want.shape), want, tol, "vae_input")
    print(f"vae_input B {B} HW {HW}: largest error / bound {r:.3f}")
    assert untouched(out[want.size:])


@pytest.mark.parametrize("mode", ["both", "mode", "moments_only", "z_only"])
@pytest.mark.parametrize("B,HW", ks.VAE_MOMENTS_SHAPES)
def test_vae_moments(B, HW, mode):
    """quant_conv + the posterior sample: both outputs under eps; eps NULL (the mode); the moments alone; z alone.
    MI355X: largest error / bound, moments 0.17, z 0.12"""
    a = ks.vae_moments_case(B, HW)
    eps = None if mode == "mode" else a["eps"]
    lv = ks.vae_moments_ref(a["h"], a["w"], a["b"], eps, B, HW)[0][:, 4:]
    assert (lv < -30).any() and (lv > 20).any() and ((lv > -30) & (lv < 20)).any()
    c = ks.ctx()
    mo = None if mode == "z_only" else np.zeros(B * 8 * HW + VAE_TAIL, np.float32)
    z = None if mode == "moments_only" else np.zeros(B * 4 * HW + VAE_TAIL, np.float32)
    c.check(c.lib.dd_dev_vae_moments(c.handle, B, HW, P(a["h"]), P(a["w"]), P(a["b"]), P(eps), P(mo), P(z), None))
    m64, tol_m, z64, tol_z = ks.vae_moments_ref(a["h"], a["w"], a["b"], eps, B, HW)
    if mo is not None:
        r = gate(mo[:m64.size].reshape(m64.shape), m64, tol_m, "moments")
        print(f"vae_moments {mode} B {B} HW {HW}: moments largest error / bound {r:.3f}")
        assert untouched(mo[m64.size:])
    if z is not None:
        r = gate(z[:z64.size].reshape(z64.shape), z64, tol_z, "z")
        print(f"vae_moments {mode} B {B} HW {HW}: z largest error / bound {r:.3f}")
        assert untouched(z[z64.size:])
    if mode == "both":
        with pytest.raises(ValueError):
            c.check(c.lib.dd_dev_vae_moments(c.handle, B, HW, P(a["h"]), P(a["w"]), P(a["b"]), P(eps), None, None, None))


# ---------------------------------------------------------------- softmax
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("rows,n", ks.SOFTMAX_SHAPES)
def test_softmax_rows(rows, n, prec):
    """softmax(scale s) per row, scale = 1 / sqrt(512).  MI355X: largest error / bound fp32 0.15, bf16 0.50"""
    s = ks.softmax_inputs(rows, n)
    out = ks.run_softmax(prec, rows, n, ks.SOFTMAX_SCALE, s)
    want, tol = ks.softmax_ref(s, ks.SOFTMAX_SCALE, prec)
    r = gate(values(out[:rows * n], prec).reshape(rows, n), want, tol, "softmax")
    print(f"softmax {prec} rows {rows} n {n}: largest error / bound {r:.3f}")
    assert untouched(out[rows * n:])
    if rows > 1 and n > 1:
        assert want[1, -1] == 1.0 and (want[1, :-1] < 2.0 ** -126).all()      # the dominant entry: everything else underflows


# ---------------------------------------------------------------- GroupNorm
def _groupnorm(prec, B, HW, C, swish, const=False):
    case = ks.gn_case(B, HW, C, swish, const)
    out, part = ks.run_groupnorm(prec, B, HW, C, swish, case["x"], case["gamma"], case["beta"])
    n = B * HW * C
    got = values(out[:n], prec).astype(np.float64).reshape(B * HW, C)
    assert untouched(out[n:]) and untouched(part[-VAE_TAIL:]) and np.isfinite(part[:-VAE_TAIL]).all()
    return case, got


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("swish", [0, 1])
@pytest.mark.parametrize("B,HW,C", ks.GN_SHAPES)
def test_groupnorm(B, HW, C, swish, prec):
    """Each (image, group) has one of the (mean, std) pairs (0, 1), (10, 1), (100, 1), (30, 0.1), rotated by the image.
    MI355X, fp32: largest err / e32 per pair 2.81, 0.83, 0.56, 0.65 (bound 8).  The one-pass statistics this replaced (sums of x and x^2 in
    fp32): 1.58, 29.0, 410, 1567 on the same inputs."""
    case, got = _groupnorm(prec, B, HW, C, swish)
    err = np.abs(got - case["want"])
    if prec == "fp32":
        per = [float((err / case["e32"])[case["cls"] == k].max()) for k in range(len(ks.GN_PAIRS))]
        print(f"groupnorm fp32 B {B} HW {HW} C {C} swish {swish}: err / e32 per (mean, std) pair " + " ".join(f"{v:.2f}" for v in per) +
              f" (bound {ks.GN_MARGIN:g}); e32 of the case {case['e32_case']:.3e}, err / that {err.max() / case['e32_case']:.2f}")
    r = gate(got, case["want"], ks.gn_tol(case, prec), "groupnorm")
    print(f"groupnorm {prec} B {B} HW {HW} C {C} swish {swish}: largest error / bound {r:.3f}")


@pytest.mark.parametrize("prec", PRECS)
def test_groupnorm_constant_group(prec):
    """a group that holds one value that is no short binary fraction: finite output, y = beta within the bound (rstd = 1000)"""
    B, HW, C = 2, 64, 128
    case, got = _groupnorm(prec, B, HW, C, 0, const=True)
    assert np.isfinite(got).all()
    tol = ks.gn_tol(case, prec).copy()
    cpg = C // 32
    for b, g in ((0, 7), (B - 1, 5)):
        sl = (slice(b * HW, (b + 1) * HW), slice(g * cpg, (g + 1) * cpg))
        x, gamma, beta = case["x"][sl].astype(np.float64), case["gamma"][sl[1]].astype(np.float64), case["beta"][sl[1]].astype(np.float64)
        t = ks.GN_MARGIN * case["e32_case"] + np.abs(gamma) * 1000.0 * 8 * ks.U24 * np.abs(x)
        tol[sl] = t + (ks.ulp_bf16(beta) if prec == "bf16" else 0.0)
        assert (np.abs(got[sl] - beta) <= tol[sl]).all()
    gate(got, case["want"], tol, "groupnorm, constant groups")


def test_groupnorm_batch_independence():
    """an image normalises the same alone as in a batch, bit for bit (the statistics, their pivot included, are per image)"""
    B, HW, C = 3, 300, 512
    case = ks.gn_case(B, HW, C, 1)
    whole, _ = ks.run_groupnorm("fp32", B, HW, C, 1, case["x"], case["gamma"], case["beta"])
    for b in (0, 2):
        alone, _ = ks.run_groupnorm("fp32", 1, HW, C, 1, case["x"][b * HW:(b + 1) * HW], case["gamma"], case["beta"])
        assert np.array_equal(alone[:HW * C].view(np.uint32), whole[b * HW * C:(b + 1) * HW * C].view(np.uint32)), b


@pytest.mark.parametrize("C", [64, 1152])
def test_groupnorm_refuses(C):
    c = ks.ctx()
    x, g = np.zeros(4 * C, np.float32), np.zeros(C, np.float32)
    out = np.zeros(4 * C + VAE_TAIL, np.float32)
    with pytest.raises(UNSUPPORTED, match="groupnorm"):
        c.check(c.lib.dd_dev_groupnorm(c.handle, ks.PREC_FP32, 1, 4, C, 0, P(x), P(g), P(g), P(out), None, None))
    assert not out.any()
