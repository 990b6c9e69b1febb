"""GPU unit tests of the plain attention launch (csrc/attention.hip attention_kernel<T, 9> for L = 257 / 258, attention_kernel<T, 0> for any
other L <= 288; T = bf16 and fp32) through its development entry point dd_dev_attention (include/duodiff_dev.h), against a float64
softmax(q k^T / 8) v of the SAME operands (bf16 mode: q, k, v rounded to bf16 first, so they are exact).  Replaces reference
models/uvit.py:155-164.  The shipped 512 / 768 / 1024 models take qkv_attention_kernel (tests/test_qkv_attention.py); this kernel runs in the
fp32 engine, in the small-width models and under DD_DEV_NO_FUSED_QA, and the whole-model gates dilute what it can get wrong.

The gates are per element, in units of A = P . |V| (the softmax weights times the magnitudes they multiply: the scale of the result):
  * bf16: |got - want| <= 1.75 x 2^-8 A.  P is rounded to bf16 before the P . V product and the output is rounded to bf16.  A bf16 rounding is
    2^-9 relative in the middle of a binade but 2^-8 at its lower end (8 significant bits), so the two roundings together are at most 2 x 2^-8 A.
    With scores spread over a few units (sigma 1.5) a CPU emulation of exactly that arithmetic (emulate_bf16) stays near 1.0 - 1.3 units; with a
    nearly one-hot softmax (sigma 4: one weight and the output decide everything) it reaches 1.670 units on these cases, and so does the
    kernel (1.670, same case).  The margin first set here, 1.5, therefore cannot hold for correct arithmetic; 1.75 is the smallest quarter
    step that does, and 2 or more would be a bug, not rounding.
  * fp32: |got - want| <= max(8 e32, 2^-20) A, e32 = the largest |emul - want| / A of a numpy-float32 evaluation of the same formula for the
    case (computed here, from the reference and not from the kernel); the 8 is for summation order.
Exact properties: every output is finite although the pad rows [L, Lp) of the head-major buffer hold NaN; the 8 canary rows behind the output
are untouched; an image's result does not depend on the batch it rides in; refused shapes return an error and write nothing.
test_gates_reject_the_bugs_they_are_meant_to_catch (CPU, no GPU mark) feeds corrupted references to the same gate.
"""
import ctypes as C

import numpy as np
import pytest

from kernel_support import PREC_BF16, PREC_FP32, bf16, from_bf16_bits, gate

gpu = pytest.mark.gpu

PREC_NAME = {PREC_BF16: "bf16", PREC_FP32: "fp32"}
BF16_UNIT = 2.0 ** -8          # bf16 P in the P . V product + the bf16 output rounding, relative to A
BF16_MARGIN = 1.75             # the two roundings at the lower end of a binade (at most 2), v_exp_f32, accumulation order
FP32_MARGIN = 8.0              # summation order, relative to the numpy-float32 evaluation's own error
FP32_FLOOR = 2.0 ** -20


# ---------------------------------------------------------------------------------------------------------------- host helpers
def operands(B, H, L, sigma, seed, prec, big_keys=()):
    """q, k [B, H, L, 64] of standard deviation sigma (scores q . k / 8 of standard deviation sigma^2: 1.5 spreads them over a few units, 4 makes
    the softmax nearly one-hot), v of 1; big_keys: key rows made 3 x larger.  bf16 mode: rounded, so the kernel's operands are exact."""
    r = np.random.default_rng(seed)
    q = (sigma * r.standard_normal((B, H, L, 64))).astype(np.float32)
    k = (sigma * r.standard_normal((B, H, L, 64))).astype(np.float32)
    v = r.standard_normal((B, H, L, 64)).astype(np.float32)
    for j in big_keys:
        k[:, :, j] *= 3.0
    return tuple(bf16(a) if prec == PREC_BF16 else a for a in (q, k, v))


def softmax_weights(q, k):
    s = q.astype(np.float64) @ k.astype(np.float64).transpose(0, 1, 3, 2) * 0.125
    p = np.exp(s - s.max(-1, keepdims=True))
    return p / p.sum(-1, keepdims=True)


def reference(q, k, v):
    """float64 (want, A) as [B, H, L, 64]"""
    p = softmax_weights(q, k)
    return p @ v.astype(np.float64), p @ np.abs(v.astype(np.float64))


def emulate_fp32(q, k, v):
    """the same formula in numpy float32"""
    s = (q @ k.transpose(0, 1, 3, 2)) * np.float32(0.125)
    p = np.exp(s - s.max(-1, keepdims=True))
    return (p @ v) / p.sum(-1, keepdims=True)


def emulate_bf16(q, k, v):
    """the bf16 kernel's two roundings and nothing else: P to bf16 in front of the P . V product (the sum of P is not rounded), the result to bf16"""
    s = q.astype(np.float64) @ k.astype(np.float64).transpose(0, 1, 3, 2) * 0.125
    p = np.exp(s - s.max(-1, keepdims=True))
    o = (bf16(p.astype(np.float32)).astype(np.float64) @ v.astype(np.float64)) / p.sum(-1, keepdims=True)
    return bf16(o.astype(np.float32))


def rows(a):
    """[B, H, L, 64] -> [B L, 64 H]: "B H L D -> B L (H D)" """
    B, H, L, _ = a.shape
    return a.transpose(0, 2, 1, 3).reshape(B * L, 64 * H)


def tolerance(prec, q, k, v, want, A):
    """the per-element bound of the case and e32 (fp32 mode)"""
    if prec == PREC_BF16:
        return BF16_MARGIN * BF16_UNIT * A, None
    e32 = float((np.abs(emulate_fp32(q, k, v).astype(np.float64) - want) / A).max())
    return max(FP32_MARGIN * e32, FP32_FLOOR) * A, e32


# ---------------------------------------------------------------------------------------------------------------- GPU call
def run_attention(prec, q, k, v):
    """dd_dev_attention; returns (the whole output buffer [B L + 8, 64 H] as stored: bf16 bits or fp32)"""
    from duodiff_amd.engine import Context
    ctx = Context.get()
    B, H, L, _ = q.shape
    out = np.full((B * L + 8, 64 * H), 0xA5A5 if prec == PREC_BF16 else 0xA5A5A5A5, np.uint16 if prec == PREC_BF16 else np.uint32)
    q, k, v = (np.ascontiguousarray(a, np.float32) for a in (q, k, v))
    st = ctx.lib.dd_dev_attention(ctx.handle, prec, B, L, H, q.ctypes.data, k.ctypes.data, v.ctypes.data, out.ctypes.data, 0, None,
                                  C.byref(C.c_float(0)))
    ctx.check(st)
    return out


def check_case(prec, B, H, L, sigma, seed, big_keys=()):
    q, k, v = operands(B, H, L, sigma, seed, prec, big_keys)
    want, A = reference(q, k, v)
    tol, e32 = tolerance(prec, q, k, v, want, A)
    out = run_attention(prec, q, k, v)
    body, canary = out[: B * L], out[B * L:]
    assert np.all(canary == (0xFFFF if prec == PREC_BF16 else 0xFFFFFFFF)), "the rows behind the output were written"
    got = from_bf16_bits(body) if prec == PREC_BF16 else body.view(np.float32)
    assert np.isfinite(got).all(), "a NaN pad row of the head-major buffer reached the output"
    what = f"attention {PREC_NAME[prec]} B={B} H={H} L={L} sigma={sigma} big_keys={tuple(big_keys)}"
    rel = float((np.abs(got.astype(np.float64) - rows(want)) / rows(A)).max())      # printed before the gate asserts
    if prec == PREC_BF16:
        print(f"{what}: max |err| / A = {rel / BF16_UNIT:.3f} x 2^-8 (bound {BF16_MARGIN})")
    else:
        print(f"{what}: max |err| / A = {rel:.3e} = {rel / max(e32, 1e-300):.2f} x e32 ({e32:.3e}; bound {FP32_MARGIN} x e32, floor 2^-20)")
    gate(got, rows(want), rows(tol), what)
    return got


# L on attention_kernel<T, 0> (one key in the last tile, 31 keys, exact multiples of 32, the largest L) and 257 / 258 on <T, 9>;
# (B, H) over {(3, 1), (2, 2), (1, 8), (2, 12)} with L = 257 and L = 65 at H = 12; B H <= 48
SHAPES = [(1, 3, 1), (8, 2, 2), (17, 1, 8), (31, 3, 1), (32, 2, 2), (33, 1, 8), (64, 3, 1), (65, 2, 12), (255, 2, 2), (256, 1, 8), (259, 3, 1),
          (288, 2, 2), (257, 2, 12), (258, 1, 8), (257, 3, 1), (258, 2, 2)]


@gpu
@pytest.mark.parametrize("sigma", [1.5, 4.0])
@pytest.mark.parametrize("L,B,H", SHAPES)
@pytest.mark.parametrize("prec", [PREC_BF16, PREC_FP32], ids=["bf16", "fp32"])
def test_attention_against_float64_reference(prec, L, B, H, sigma):
    check_case(prec, B, H, L, sigma, seed=1000 * L + 10 * H + B)


@gpu
@pytest.mark.parametrize("big_keys", [(0, 1), (256, 257)])
@pytest.mark.parametrize("prec", [PREC_BF16, PREC_FP32], ids=["bf16", "fp32"])
def test_attention_where_two_keys_carry_most_of_the_mass(prec, big_keys):
    """L = 258 with two keys 3 x larger than the rest, so that they take most of the softmax mass of the queries they align with: keys 0 and 1
    (the extra tokens of a label-conditional model) and keys 256 and 257, which in this kernel's token order are the two real keys of the 9th tile
    -- every query's sum then rests on the two registers that attend_tiles keeps of that tile."""
    B, H, L = 2, 2, 258
    q, k, v = operands(B, H, L, 1.5, 77, prec, big_keys)
    mass = softmax_weights(q, k)[..., list(big_keys)].sum(-1)
    print(f"keys {big_keys}: mass on them: median {np.median(mass):.3f}, above one half for {float((mass > 0.5).mean()):.2f} of the queries")
    check_case(prec, B, H, L, 1.5, 77, big_keys)


@gpu
@pytest.mark.parametrize("L", [33, 65, 257, 258])
@pytest.mark.parametrize("prec", [PREC_BF16, PREC_FP32], ids=["bf16", "fp32"])
def test_an_image_does_not_depend_on_its_batch(prec, L):
    """image b of a B = 3 call is bit-equal to a B = 1 call on that image"""
    B, H = 3, 2
    q, k, v = operands(B, H, L, 1.5, 5 + L, prec)
    whole = run_attention(prec, q, k, v)
    for b in range(B):
        one = run_attention(prec, q[b:b + 1], k[b:b + 1], v[b:b + 1])
        assert np.array_equal(whole[b * L:(b + 1) * L], one[:L]), (L, b)


@gpu
@pytest.mark.parametrize("prec", [PREC_BF16, PREC_FP32], ids=["bf16", "fp32"])
def test_refused_shapes_return_an_error_and_write_nothing(prec):
    """L = 0, L = 289 and whatever else the launcher or the entry point refuses: an error code, no launch, the output array as the caller left it"""
    from duodiff_amd import _lib
    from duodiff_amd.engine import Context
    ctx = Context.get()
    for B, H, L in [(1, 2, 0), (1, 2, 289), (2, 1, 320), (1, 2, -1), (0, 2, 17), (1, 0, 17)]:
        z = np.zeros((max(B, 1), max(H, 1), max(L, 1), 64), np.float32)
        out = np.full((max(B, 1) * max(L, 1) + 8, 64 * max(H, 1)), 0xA5A5A5A5, np.uint32)
        st = ctx.lib.dd_dev_attention(ctx.handle, prec, B, L, H, z.ctypes.data, z.ctypes.data, z.ctypes.data, out.ctypes.data, 0, None,
                                      C.byref(C.c_float(0)))
        assert st in (_lib.DD_ERR_INVALID, _lib.DD_ERR_UNSUPPORTED), (B, H, L, st)
        assert np.all(out == 0xA5A5A5A5), (B, H, L)


# ---------------------------------------------------------------------------------------------------------------- the gates themselves (CPU)
def test_gates_reject_the_bugs_they_are_meant_to_catch():
    """The gates above, applied to float64 references corrupted the way this kernel can go wrong, reject each under the bf16 and the fp32 bound:
    the last valid key left out; one padded key taking part with score 0 (K and V rows of zeros, what the fp32 staging holds there); keys 256 and
    257 swapped in V only; the split chunk's four partial results merged without the exp(m_w - M) rescaling; the two d-halves of a head swapped.
    (A score-0 key weighs exp(-max score) of the largest weight: under the bf16 bound it shows where the sequence is short, L = 17 here; at
    L = 258 only the fp32 bound can see it, and is asserted to.)"""
    def both_gates(q32, k32, v32):
        for prec in (PREC_BF16, PREC_FP32):
            q, k, v = (bf16(a) if prec == PREC_BF16 else a for a in (q32, k32, v32))
            want, A = reference(q, k, v)
            tol, _ = tolerance(prec, q, k, v, want, A)
            yield prec, q.astype(np.float64), k.astype(np.float64), v.astype(np.float64), want, tol

    def rejects(bad, want, tol, what):
        with pytest.raises(AssertionError):
            gate(bad, want, tol, what)

    def softmax_v(s, v):
        p = np.exp(s - s.max(-1, keepdims=True))
        return (p @ v) / p.sum(-1, keepdims=True)

    B, H, L = 2, 2, 258
    q32, k32, v32 = operands(B, H, L, 1.5, 3, PREC_FP32)
    for prec, q, k, v, want, tol in both_gates(q32, k32, v32):
        name = PREC_NAME[prec]
        s = q @ k.transpose(0, 1, 3, 2) * 0.125
        # what a correct kernel returns passes: the reference rounded to the output type (and the float32 evaluation under the fp32 bound)
        if prec == PREC_BF16:
            assert gate(bf16(want.astype(np.float32)), want, tol, "bf16 of the reference") < 1.0
        else:
            assert gate(want.astype(np.float32), want, tol, "fp32 of the reference") < 1.0
            assert gate(emulate_fp32(q32, k32, v32), want, tol, "float32 evaluation") <= 1.0 / FP32_MARGIN + 1e-12
        rejects(softmax_v(s[..., :L - 1], v[:, :, :L - 1]), want, tol, f"{name}: last valid key left out")
        vs = v.copy()
        vs[:, :, [256, 257]] = v[:, :, [257, 256]]
        rejects(softmax_v(s, vs), want, tol, f"{name}: keys 256 and 257 swapped in V")
        # the split chunk (queries 256, 257): wave w holds key tiles w, w + 4 (wave 3: and the 9th); merged as if all four maxima were equal
        bad = want.copy()
        tiles = np.arange(L) // 32
        num, den = 0.0, 0.0
        for w in range(4):
            keys = np.flatnonzero((tiles == w) | (tiles == w + 4) | ((tiles == 8) & (w == 3)))
            sw = s[:, :, 256:, :][..., keys]
            pw = np.exp(sw - sw.max(-1, keepdims=True))
            num, den = num + pw @ v[:, :, keys], den + pw.sum(-1, keepdims=True)
        bad[:, :, 256:] = num / den
        rejects(bad, want, tol, f"{name}: partials merged without rescaling")
        rejects(np.concatenate([want[..., 32:], want[..., :32]], -1), want, tol, f"{name}: d-halves swapped")
        if prec == PREC_FP32:
            s0 = np.concatenate([s, np.zeros_like(s[..., :1])], -1)
            v0 = np.concatenate([v, np.zeros_like(v[:, :, :1])], 2)
            rejects(softmax_v(s0, v0), want, tol, "fp32: one padded key with score 0 at L = 258")
    # the bf16 margin: the two roundings alone, on a nearly one-hot softmax, pass it and exceed 1.5 units (a case of the GPU test)
    q, k, v = operands(1, 8, 17, 4.0, 1000 * 17 + 10 * 8 + 1, PREC_BF16)
    want, A = reference(q, k, v)
    units = gate(emulate_bf16(q, k, v), want, tolerance(PREC_BF16, q, k, v, want, A)[0], "emulated bf16 arithmetic") * BF16_MARGIN
    assert 1.5 < units < 2.0, units
    q32, k32, v32 = operands(3, 1, 17, 1.5, 4, PREC_FP32)
    for prec, q, k, v, want, tol in both_gates(q32, k32, v32):
        s = q @ k.transpose(0, 1, 3, 2) * 0.125
        s0 = np.concatenate([s, np.zeros_like(s[..., :1])], -1)
        v0 = np.concatenate([v, np.zeros_like(v[:, :, :1])], 2)
        rejects(softmax_v(s0, v0), want, tol, f"{PREC_NAME[prec]}: one padded key with score 0 at L = 17")
        rejects(softmax_v(s[..., :16], v[:, :, :16]), want, tol, f"{PREC_NAME[prec]}: last valid key left out at L = 17")
