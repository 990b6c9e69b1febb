"""GPU unit tests of the streaming attention launch for long sequences (csrc/attention.hip attention_long_kernel<T>, T = bf16 and fp32; the model
takes it where L > 288) through its development entry point dd_dev_attention_long (include/duodiff_dev.h), against the float64
softmax(q k^T / 8) v of tests/test_attention.py on the same operands.  K and V go through LDS in key blocks of KB = 288 keys, a workgroup holds
a slab of 128 queries, and a query's result is merged across the blocks by the online softmax (running maximum, running sum, rescaled
accumulator, fp32).

The gates are those of tests/test_attention.py, imported and unchanged: per element, in units of A = P . |V|,
  * bf16: |got - want| <= 1.75 x 2^-8 A.  The derivation carries over: P is rounded to bf16 once per key block, relative to that block's own
    maximum (a relative rounding, so the rescaling by exp(m_b - M) <= 1 in fp32 does not change its size relative to A), and the output is
    rounded once.  test_blockwise_bf16_arithmetic_passes_the_gate (CPU) emulates exactly that arithmetic in numpy -- P rounded per block
    against the block's maximum, float64 merge, one output rounding -- and asserts that it passes the gate on every bf16 case sent to the GPU.
  * fp32: |got - want| <= max(8 e32, 2^-20) A, e32 from the numpy-float32 evaluation of the case.
Shapes: L = 1, 33, 288 (valid for the old kernel too), 289 = KB + 1, 2 KB - 1, 2 KB, 2 KB + 1, 383 / 384 / 385 (a multiple of the query slab and
its neighbours), 325 and 578 (the whole-model tests' lengths), 1025 / 1026 (1024 patches), 4098 (the limit); (B, H) over {(3, 1), (2, 2), (1, 8)},
one case at H = 16.  Exact properties: finite outputs although the pad rows hold NaN; untouched canary rows; an image does not depend on its
batch; refused shapes write nothing.  test_gates_reject_what_a_streaming_kernel_can_get_wrong (CPU) feeds corrupted references to the gate.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from kernel_support import PREC_BF16, PREC_FP32, bf16, from_bf16_bits, gate
from test_attention import BF16_MARGIN, BF16_UNIT, FP32_MARGIN, PREC_NAME, operands, reference, rows, run_attention, tolerance

gpu = pytest.mark.gpu

KB = 288           # keys per key block (9 tiles of 32)
SLAB = 128         # queries per workgroup


@functools.lru_cache(maxsize=None)
def case(prec, B, H, L, sigma, seed, big_keys=()):
    """(q, k, v, want, A, tol, e32) of a case, computed once for the tests that share it and never modified"""
    q, k, v = operands(B, H, L, sigma, seed, prec, big_keys)
    want, A = reference(q, k, v)
    tol, e32 = tolerance(prec, q, k, v, want, A)
    for a in (q, k, v, want, A, tol):
        a.setflags(write=False)
    return q, k, v, want, A, tol, e32


def emulate_bf16_blocks(q, k, v):
    """the bf16 kernel's roundings and nothing else: per key block P = exp(s - the block's own maximum) rounded to bf16 in front of P . V (the
    block's sum of P is not rounded), the blocks merged in float64 with exp(m_b - M), the result rounded to bf16"""
    s = q.astype(np.float64) @ k.astype(np.float64).transpose(0, 1, 3, 2) * 0.125
    v = v.astype(np.float64)
    L = s.shape[-1]
    M = s.max(-1, keepdims=True)
    num, den = 0.0, 0.0
    for k0 in range(0, L, KB):
        sb = s[..., k0:k0 + KB]
        mb = sb.max(-1, keepdims=True)
        p = np.exp(sb - mb)
        f = np.exp(mb - M)
        num = num + f * (bf16(p.astype(np.float32)).astype(np.float64) @ v[:, :, k0:k0 + KB])
        den = den + f * p.sum(-1, keepdims=True)
    return bf16((num / den).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------- GPU call
def run_attention_long(prec, q, k, v):
    """dd_dev_attention_long; returns the whole output buffer [B L + 8, 64 H] as stored: bf16 bits or fp32"""
    from duodiff_amd.engine import Context
    ctx = Context.get()
    B, H, L, _ = q.shape
    out = np.full((B * L + 8, 64 * H), 0xA5A5 if prec == PREC_BF16 else 0xA5A5A5A5, np.uint16 if prec == PREC_BF16 else np.uint32)
    q, k, v = (np.ascontiguousarray(a, np.float32) for a in (q, k, v))
    st = ctx.lib.dd_dev_attention_long(ctx.handle, prec, B, L, H, q.ctypes.data, k.ctypes.data, v.ctypes.data, out.ctypes.data, 0, None,
                                       C.byref(C.c_float(0)))
    ctx.check(st)
    return out


def values(prec, body):
    return from_bf16_bits(body) if prec == PREC_BF16 else body.view(np.float32)


def check_case(prec, B, H, L, sigma, seed, big_keys=()):
    q, k, v, want, A, tol, e32 = case(prec, B, H, L, sigma, seed, tuple(big_keys))
    out = run_attention_long(prec, q, k, v)
    body, canary = out[: B * L], out[B * L:]
    assert np.all(canary == (0xFFFF if prec == PREC_BF16 else 0xFFFFFFFF)), "the rows behind the output were written"
    got = values(prec, body)
    assert np.isfinite(got).all(), "a NaN pad row of the head-major buffer reached the output"
    what = f"attention_long {PREC_NAME[prec]} B={B} H={H} L={L} sigma={sigma} big_keys={tuple(big_keys)}"
    rel = float((np.abs(got.astype(np.float64) - rows(want)) / rows(A)).max())      # printed before the gate asserts
    if prec == PREC_BF16:
        print(f"{what}: max |err| / A = {rel / BF16_UNIT:.3f} x 2^-8 (bound {BF16_MARGIN})")
    else:
        print(f"{what}: max |err| / A = {rel:.3e} = {rel / max(e32, 1e-300):.2f} x e32 ({e32:.3e}; bound {FP32_MARGIN} x e32, floor 2^-20)")
    gate(got, rows(want), rows(tol), what)
    return got


def seed_of(L, B, H):
    return 1000 * L + 10 * H + B


SHAPES = [(1, 3, 1), (33, 2, 2), (288, 1, 8), (KB + 1, 3, 1), (KB + 1, 1, 16), (2 * KB - 1, 2, 2), (2 * KB, 1, 8), (2 * KB + 1, 3, 1),
          (3 * SLAB - 1, 2, 2), (3 * SLAB, 3, 1), (3 * SLAB + 1, 1, 8), (325, 3, 1), (578, 2, 2), (1025, 1, 8), (1026, 2, 2), (4098, 1, 1)]
SIGMAS = [1.5, 4.0]
# 16 / 24 keys 3 x larger than the rest, in the first key block only and in the last only, of three blocks (L = 600: keys 0 .. 287, 288 .. 575, 576 .. 599):
# the running maximum of most queries is set by the first block and never raised, or raised by the very last block
MASS_L, MASS_B, MASS_H, MASS_SEED = 600, 2, 2, 77
MASS_KEYS = [tuple(range(5, KB, 18)), tuple(range(2 * KB, MASS_L))]


@gpu
@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("L,B,H", SHAPES)
@pytest.mark.parametrize("prec", [PREC_BF16, PREC_FP32], ids=["bf16", "fp32"])
def test_attention_long_against_float64_reference(prec, L, B, H, sigma):
    check_case(prec, B, H, L, sigma, seed_of(L, B, H))


@gpu
@pytest.mark.parametrize("L", [33, 257, 288])
@pytest.mark.parametrize("prec", [PREC_BF16, PREC_FP32], ids=["bf16", "fp32"])
def test_the_two_kernels_agree_where_both_are_valid(prec, L):
    """the same operands through dd_dev_attention: both outputs are within the gate of float64, and of each other -- a layout mix-up in the new
    launch would show here without a reference"""
    B, H = 2, 2
    q, k, v, want, A, tol, _ = case(prec, B, H, L, 1.5, seed_of(L, B, H))
    new = check_case(prec, B, H, L, 1.5, seed_of(L, B, H))
    old = values(prec, run_attention(prec, q, k, v)[: B * L])
    gate(old, rows(want), rows(tol), f"dd_dev_attention {PREC_NAME[prec]} L={L}")
    gate(new, old.astype(np.float64), rows(tol), f"attention_long against attention_kernel, {PREC_NAME[prec]} L={L}")


@gpu
@pytest.mark.parametrize("big_keys", MASS_KEYS)
@pytest.mark.parametrize("prec", [PREC_BF16, PREC_FP32], ids=["bf16", "fp32"])
def test_attention_long_where_one_key_block_carries_the_mass(prec, big_keys):
    q, k, _, _, _, _, _ = case(prec, MASS_B, MASS_H, MASS_L, 1.5, MASS_SEED, big_keys)
    s = q.astype(np.float64) @ k.astype(np.float64).transpose(0, 1, 3, 2) * 0.125
    first = s.argmax(-1) // KB == big_keys[0] // KB
    print(f"keys {big_keys}: the maximum score lies in their block for {float(first.mean()):.2f} of the queries")
    assert first.mean() > 0.5
    check_case(prec, MASS_B, MASS_H, MASS_L, 1.5, MASS_SEED, big_keys)


@gpu
@pytest.mark.parametrize("L", [KB + 1, 2 * KB + 1])
@pytest.mark.parametrize("prec", [PREC_BF16, PREC_FP32], ids=["bf16", "fp32"])
def test_an_image_does_not_depend_on_its_batch(prec, L):
    """image b of a B = 3 call is bit-equal to a B = 1 call on that image"""
    B, H = 3, 2
    q, k, v = operands(B, H, L, 1.5, 5 + L, prec)
    whole = run_attention_long(prec, q, k, v)
    for b in range(B):
        one = run_attention_long(prec, q[b:b + 1], k[b:b + 1], v[b:b + 1])
        assert np.array_equal(whole[b * L:(b + 1) * L], one[:L]), (L, b)


@gpu
@pytest.mark.parametrize("prec", [PREC_BF16, PREC_FP32], ids=["bf16", "fp32"])
def test_refused_shapes_return_an_error_and_write_nothing(prec):
    from duodiff_amd import _lib
    from duodiff_amd.engine import Context
    ctx = Context.get()
    for B, H, L in [(1, 2, 0), (1, 2, -1), (1, 1, 4099), (0, 2, 17), (1, 0, 17)]:
        z = np.zeros((max(B, 1), max(H, 1), max(L, 1), 64), np.float32)
        out = np.full((max(B, 1) * max(L, 1) + 8, 64 * max(H, 1)), 0xA5A5A5A5, np.uint32)
        st = ctx.lib.dd_dev_attention_long(ctx.handle, prec, B, L, H, z.ctypes.data, z.ctypes.data, z.ctypes.data, out.ctypes.data, 0, None,
                                           C.byref(C.c_float(0)))
        assert st in (_lib.DD_ERR_INVALID, _lib.DD_ERR_UNSUPPORTED), (B, H, L, st)
        assert np.all(out == 0xA5A5A5A5), (B, H, L)


# ---------------------------------------------------------------------------------------------------------------- the bound and the gate (CPU)
BF16_CASES = [(B, H, L, sigma, seed_of(L, B, H), ()) for L, B, H in SHAPES for sigma in SIGMAS] + \
             [(2, 2, L, 1.5, seed_of(L, 2, 2), ()) for L in (257, 288)] +[(MASS_B, MASS_H, MASS_L, 1.5, MASS_SEED, bk) for bk in MASS_KEYS]


@pytest.mark.parametrize("B,H,L,sigma,seed,big_keys", BF16_CASES)
def test_blockwise_bf16_arithmetic_passes_the_gate(B, H, L, sigma, seed, big_keys):
    """the bound is fair: the block-wise bf16 arithmetic alone (emulate_bf16_blocks) passes the bf16 gate on every case the GPU tests send"""
    q, k, v, want, A, tol, _ = case(PREC_BF16, B, H, L, sigma, seed, big_keys)
    units = gate(emulate_bf16_blocks(q, k, v), want, tol, f"emulated block-wise bf16 arithmetic L={L} sigma={sigma}") * BF16_MARGIN
    print(f"B={B} H={H} L={L} sigma={sigma} big_keys={big_keys}: emulation at {units:.3f} x 2^-8 A (bound {BF16_MARGIN})")


def test_gates_reject_what_a_streaming_kernel_can_get_wrong():
    """The gates above, applied to float64 references corrupted the way this kernel can go wrong, reject each under the bf16 and the fp32 bound:
    one whole key block left out; two blocks merged without the exp(m_b - M) rescaling; the V rows of two blocks swapped (L = 600, three
    blocks); the last valid key left out at L = KB + 1 (it is the only key of its block).  One padded key taking part with score 0 at L = 289
    weighs exp(-max score) of the largest weight: only the fp32 bound can see it, and is asserted to."""
    def both_gates(B, H, L, seed):
        q32, k32, v32 = operands(B, H, L, 1.5, seed, PREC_FP32)
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

    L = 600
    for prec, q, k, v, want, tol in both_gates(2, 2, L, 3):
        name = PREC_NAME[prec]
        s = q @ k.transpose(0, 1, 3, 2) * 0.125
        assert gate(bf16(want.astype(np.float32)) if prec == PREC_BF16 else want.astype(np.float32), want, tol, "the reference, rounded") < 1.0
        keep = np.r_[0:KB, 2 * KB:L]
        rejects(softmax_v(s[..., keep], v[:, :, keep]), want, tol, f"{name}: the second key block left out")
        num, den = 0.0, 0.0
        for k0 in (0, KB):         # blocks 0 and 1 merged as if their maxima were equal; block 2 merged correctly behind them
            pb = np.exp(s[..., k0:k0 + KB] - s[..., k0:k0 + KB].max(-1, keepdims=True))
            num, den = num + pb @ v[:, :, k0:k0 + KB], den + pb.sum(-1, keepdims=True)
        m01 = s[..., :2 * KB].max(-1, keepdims=True)
        p2 = np.exp(s[..., 2 * KB:] - m01)
        rejects((num + p2 @ v[:, :, 2 * KB:]) / (den + p2.sum(-1, keepdims=True)), want, tol, f"{name}: two blocks merged without rescaling")
        vs = v.copy()
        vs[:, :, :KB], vs[:, :, KB:2 * KB] = v[:, :, KB:2 * KB], v[:, :, :KB]
        rejects(softmax_v(s, vs), want, tol, f"{name}: the V rows of two blocks swapped")
    L = KB + 1
    for prec, q, k, v, want, tol in both_gates(3, 1, L, 4):
        s = q @ k.transpose(0, 1, 3, 2) * 0.125
        rejects(softmax_v(s[..., :L - 1], v[:, :, :L - 1]), want, tol, f"{PREC_NAME[prec]}: last valid key left out at L = KB + 1")
        if prec == PREC_FP32:
            s0 = np.concatenate([s, np.zeros_like(s[..., :1])], -1)
            v0 = np.concatenate([v, np.zeros_like(v[:, :, :1])], 2)
            rejects(softmax_v(s0, v0), want, tol, "fp32: one padded key with score 0 at L = 289")
