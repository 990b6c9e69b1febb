"""Unit tests of the attention launch that computes attn.qkv itself (csrc/attention.hip qkv_attention_kernel<512 | 768 | 1024>: the attention
launch of every shipped bf16 model) through its development entry points dd_dev_qkv_attention_rows and dd_dev_qkv_attention
(include/duodiff_dev.h), against float64: qkv = Linear(h), q, k, v rounded to bf16 (as the stored qkv tensor of the plain path is),
softmax(q k^T / 8) v per (image, head).  Replaces reference models/uvit.py:152-164 for D = 512 / 768 / 1024, L = 256 + 1 or 2.

Operands on an exact grid.  h = clip(rint(2 N(0, 1)), -8, 8) / 2; the q and k blocks of wqkv = rint(N(0, 1) s 64) / 64 with
s = spread / (sqrt(D) std(h)), the v block the same with s = 1 / sqrt(D); bias = rint(0.3 N(0, 1) 128) / 128.  Every value is exact in bf16 and
every product and partial sum of h . w^T + bias is a multiple of 2^-7 (2^-8 where h carries quarters: the norm1 cases) far below 2^24 of those
units, so fp32 accumulation is exact IN ANY ORDER -- on the MFMA path and in the extra tokens' partial sums through LDS alike -- and the kernel's
q, k, v are bit for bit bf16(float64 qkv).  (With random float operands the fp32-accumulated q / k / v round to another bf16 value than the
reference's in about 1 element in 2000, and one flipped v under a nearly one-hot softmax costs a whole unit of the bound below: a correct kernel
could not meet it.)  test_operands_are_exact asserts that condition for every case the GPU tests use.  What is left to bound is what
tests/test_attention.py bounds for the same attention core: P rounded to bf16 in front of P . V, and the bf16 output.

The gate is per element, |got - want| <= MARGIN x 2^-8 A with A = P . |V|.  Each of the two bf16 roundings is at most 2^-8 relative (8 significant
bits: half an ulp at the lower end of a binade), the first of P, so at most 2^-8 A, the second of the result, at most 2^-8 |out| <= 2^-8 A:
correct arithmetic stays within 2 x 2^-8 A, and a kernel beyond that is wrong.  tests/test_attention.py holds the same core to BF16_MARGIN =
1.75, the smallest quarter step above what the roundings alone (emulate_bf16, a CPU evaluation that knows nothing of the kernel) reach on ITS
cases, 1.670.  These cases have 30 times as many elements and that figure's tail goes further: spread = 1.5 (scores spread over a few units,
median largest weight 0.2) gives 0.97 - 1.61 units, spread = 4 (nearly one-hot, 0.97) 1.55 - 1.83, with 1.828 on one element of 1.6 million of
D = 768, E = 2, bias, spread 4, B = 8, and 1.807 and 1.752 on two of the dominant-token cases.  1.75 therefore cannot hold for correct arithmetic here, by the
reference's own evidence and before any kernel ran; the next quarter step is the analytic bound itself, MARGIN = 2.0, with no allowance above
it.  test_reference_alone_stays_inside_the_gate pins both facts: the emulation exceeds BF16_MARGIN and stays below 2.
Exact properties: every output is finite although the rows the kernel must not read hold NaN (the patch rows of the row-major hx buffer, or
of the fp32 residual stream in the production mode); the 8 canary rows behind the output keep their 0xFFFF; the production mode (hx = nullptr:
the kernel normalises the extra-token rows itself, what Backbone launches) is bit-identical to the hx mode given bf16(float64 LayerNorm); an
image's result does not depend on its batch nor on which of the two workgroup -> (image, head) maps placed it; refused shapes return
DD_ERR_UNSUPPORTED and write nothing.  test_gates_reject_the_bugs_they_are_meant_to_catch (CPU) feeds eight corrupted references to the gate.
Tried once on the GPU: a build whose split-chunk merge lacks the exp(m_w - M) factors failed 47 of the 50 GPU tests of this file, one with a
one-pass variance in the in-kernel norm1 all six norm1 cases and nothing else.

OBSERVED on the MI355X, max |err| / A in units of 2^-8 over the per-element, dominant-token and norm1 cases, patch rows | extra-token rows:
    D =  512: spread 1.5  1.18 - 1.36 | 0.77 - 0.96     spread 4  1.55 - 1.73 | 0.96 - 1.10
    D =  768: spread 1.5  0.97 - 1.36 | 0.74 - 1.01     spread 4  1.66 - 1.83 | 0.96 - 1.18
    D = 1024: spread 1.5  1.13 - 1.61 | 0.83 - 1.17     spread 4  1.60 - 1.81 | 0.97 - 1.29
The patch rows' figure equals the CPU emulation's to all three digits in every one of the 39 cases (the largest, 1.828, on the case where
the emulation has 1.828); the extra-token rows, whose P . V runs in fp32 partial sums over 8 waves, stay lower.  Both bit-identity tests held.

The first test, on random float operands with two global gates (max err <= 2e-2 max|out|, rms <= 3e-3), is the file's original one, unchanged.
"""
import ctypes as C

import numpy as np
import pytest

from kernel_support import bf16, from_bf16_bits, gate
from test_attention import BF16_MARGIN, BF16_UNIT, emulate_bf16, reference, rows

gpu = pytest.mark.gpu
MARGIN = 2.0          # the two bf16 roundings' analytic bound, in units of 2^-8 A (the docstring: why BF16_MARGIN = 1.75 cannot hold on these cases)
assert BF16_MARGIN < MARGIN <= 2.0
# Where the softmax is one-hot to below fp32's range AND the v element under the one weight is exactly 0 (the grid has zeros), A itself is below
# 2^-126: a P below the smallest normal fp32 may be flushed (at most 258 keys x 2^-126 x max|v| < 2^-115 in all), and so may an output below the
# smallest normal bf16 (2^-126).  The bound never goes below that: 2.4e-35, nothing on the scale of any result.
FLOOR = 2.0 ** -115


def tolerance(A):
    return np.maximum(MARGIN * BF16_UNIT * A, FLOOR)


def _reference(h, w, bias, B, L, H):
    D = 64 * H
    qkv = bf16(h).astype(np.float64) @ bf16(w).astype(np.float64).T
    if bias is not None:
        qkv = qkv + bias.astype(np.float64)
    qkv = bf16(qkv.astype(np.float32)).astype(np.float64).reshape(B, L, 3, H, 64)     # "B L (K H D) -> K B H L D"
    q, k, v = (qkv[:, :, i].transpose(0, 2, 1, 3) for i in range(3))
    s = q @ k.transpose(0, 1, 3, 2) * 0.125
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    return (p @ v).transpose(0, 2, 1, 3).reshape(B * L, D)                               # "B H L D -> B L (H D)"


@gpu
@pytest.mark.parametrize("B,extras,with_bias,H", [(3, 1, False, 8), (8, 2, False, 8), (5, 2, True, 8), (16, 1, True, 8),
                                                  (3, 2, False, 12), (8, 2, True, 12), (2, 2, True, 16), (8, 1, False, 16)])
def test_qkv_attention_against_float64_reference(B, extras, with_bias, H):
    """H = 8 / 12 / 16 = embed_dim 512 / 768 / 1024: the k range of the Linear is walked in 2 / 3 / 4 parts of 16 k-steps."""
    from duodiff_amd.engine import Context
    ctx = Context.get()
    D, L = 64 * H, 256 + extras
    g = np.random.default_rng(100 * B + extras)
    h = g.standard_normal((B * L, D), dtype=np.float32)
    # weights scaled so that the scores spread over a few units (a flat softmax would hide a wrong key order)
    w = (g.standard_normal((3 * D, D), dtype=np.float32) * (0.09 * (512.0 / D) ** 0.5)).astype(np.float32)
    bias = (g.standard_normal(3 * D, dtype=np.float32) * 0.3).astype(np.float32) if with_bias else None
    out = np.zeros((B * L, D), np.uint16)
    ms = C.c_float(0)
    ctx.check(ctx.lib.dd_dev_qkv_attention(ctx.handle, B, L, H, extras, h.ctypes.data, w.ctypes.data, bias.ctypes.data if with_bias else None,
                                           out.ctypes.data, 5, None, C.byref(ms)))
    got = (out.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    want = _reference(h, w, bias, B, L, H)
    err = np.abs(got - want)
    rows = np.arange(B * L) % L
    print(f"qkv_attention B={B} H={H} extras={extras} bias={with_bias}: max err {err.max():.3e} (patch rows {err[rows >= extras].max():.3e}, "
          f"extra rows {err[rows < extras].max():.3e}); |out| max {np.abs(want).max():.2f}; {ms.value * 1e3:.1f} us/launch")
    # bf16 output rounding (2^-9 relative) + bf16 P in the P V product + accumulation order
    assert err.max() <= 2e-2 * max(1.0, np.abs(want).max())
    assert np.sqrt((err ** 2).mean()) <= 3e-3


# ---------------------------------------------------------------------------------------------------------------- operands on the exact grid
class Case:
    """One problem: D, extras, bias on / off, spread, B, seed; doubled: the token whose row of h is doubled in every image; norm1: the
    extra-token rows come from LayerNorm of constructed residual rows (the production mode) instead of the grid."""

    def __init__(self, D, extras, with_bias, spread, B, seed, doubled=None, norm1=False):
        self.D, self.E, self.with_bias, self.spread, self.B, self.seed, self.doubled, self.norm1 = D, extras, with_bias, spread, B, seed, doubled, norm1
        self.H, self.L = D // 64, 256 + extras

    def __repr__(self):
        return (f"D={self.D} E={self.E} bias={int(self.with_bias)} spread={self.spread} B={self.B}" +
                (f" doubled={self.doubled}" if self.doubled is not None else "") + (" norm1" if self.norm1 else ""))

    def operands(self):
        """h [B L, D], wqkv [3 D, D], bias [3 D] or None (fp32, on the grid); norm1 cases: + xres [B L, D] (extra rows only; the rest NaN), ln [2, D]"""
        B, L, D, E = self.B, self.L, self.D, self.E
        r = np.random.default_rng(self.seed)
        h = (np.clip(np.rint(2.0 * r.standard_normal((B * L, D))), -8, 8) / 2).astype(np.float32)
        sd = float(h.std())

        def block(s):
            return np.rint(r.standard_normal((D, D)) * s * 64) / 64
        sqk = self.spread / (np.sqrt(D) * sd)
        w = np.concatenate([block(sqk), block(sqk), block(1.0 / np.sqrt(D))]).astype(np.float32)
        bias = (np.rint(0.3 * r.standard_normal(3 * D) * 128) / 128).astype(np.float32) if self.with_bias else None
        if self.doubled is not None:
            h.reshape(B, L, D)[:, self.doubled] *= 2
        if not self.norm1:
            return h, w, bias
        # residual rows mu + z: z a permutation of {+-0.5 on D / 2 columns, +-1 on 3 D / 8, +-2 on D / 8, signs balanced}: mean 0, variance 1 exactly
        z0 = np.repeat([0.5, -0.5, 1.0, -1.0, 2.0, -2.0], [D // 4, D // 4, 3 * D // 16, 3 * D // 16, D // 16, D // 16])
        assert z0.size == D and z0.sum() == 0 and (z0 ** 2).sum() == D
        xres = np.full((B, L, D), np.nan, np.float32)
        for i in range(B * E):
            xres[i // E, i % E] = MU[i % len(MU)] + r.permutation(z0)
        # beta: multiples of 0.25 that cancel no gamma z (+-0.25 .. +-4, powers of two) to zero -- there the eps term would be all of the result
        ln = np.stack([r.choice([0.5, 1.0, 2.0], D), r.choice([0.0, 0.75, -0.75, 1.25, -1.25, 1.5, -1.5, 1.75, -1.75], D)]).astype(np.float32)
        x = xres[:, :E].astype(np.float64)
        mean = x.mean(-1, keepdims=True)
        var = ((x - mean) ** 2).mean(-1, keepdims=True)
        h.reshape(B, L, D)[:, :E] = bf16(((x - mean) / np.sqrt(var + 1e-5) * ln[0] + ln[1]).astype(np.float32))      # bf16(float64 LayerNorm)
        return h, w, bias, xres.reshape(B * L, D), ln

    def qkv64(self, h, w, bias):
        x = h.astype(np.float64) @ w.astype(np.float64).T
        return x + bias.astype(np.float64) if bias is not None else x

    def heads(self, qkv):
        """[B L, 3 D] -> q, k, v [B, H, L, 64]: "B L (K H D) -> K B H L D" """
        t = np.asarray(qkv).reshape(self.B, self.L, 3, self.H, 64)
        return tuple(np.ascontiguousarray(t[:, :, i].transpose(0, 2, 1, 3)) for i in range(3))

    def qkv_bf16(self, h, w, bias):
        """q, k, v [B, H, L, 64] as the kernel holds them: bf16(float64 qkv)"""
        return self.heads(bf16(self.qkv64(h, w, bias).astype(np.float32)))

    def extra_rows(self):
        return (np.arange(self.B * self.L) % self.L) < self.E


# The norm1 cases' row offsets.  0, 100, -2000, 7: the mean has to be subtracted exactly.  5000, -4097: a ONE-pass variance in fp32 (mean of x^2
# minus mean^2) comes out 0 or 2 instead of 1 there (x^2 > 2^24 loses the fraction that holds the variance; test_operands_are_exact shows it); up
# to -2000 the squares of these rows are still exact in fp32, and a kernel built with a one-pass variance got 5 of the 6 cases right on those
# four offsets alone.  Each case has >= 6 extra rows.
MU = (0.0, 100.0, -2000.0, 7.0, 5000.0, -4097.0)

# (extras, bias, spread, B) at every D: every value of every axis, B = 3 / 8 on the two workgroup -> (image, head) maps
_AXES = [(1, False, 1.5, 3), (2, True, 4.0, 8), (2, False, 4.0, 3), (1, True, 1.5, 8), (2, True, 1.5, 3), (1, False, 4.0, 8), (1, True, 4.0, 3)]
PER_ELEMENT = [Case(D, E, wb, sp, B, seed=7 * D + 10 * i + B) for D in (512, 768, 1024) for i, (E, wb, sp, B) in enumerate(_AXES)]
# the doubled token: image rows 0, 37, 100, 255 = key tiles 0, 1, 3, 7 (waves 0, 1, 3, 7 of the split chunk); tokens 0 and E - 1: the 9th tile (wave 7)
DOMINANT = [Case(D, 2, True, 4.0, 3, seed=D + t, doubled=t) for D in (512, 1024) for t in (2 + 0, 2 + 37, 2 + 100, 2 + 255, 0, 1)]
NORM1 = [Case(D, E, True, 1.5, 8 if E == 1 else 3, seed=3 * D + E, norm1=True) for D in (512, 768, 1024) for E in (1, 2)]
ALL_CASES = PER_ELEMENT + DOMINANT + NORM1


def units(got, want, A, sel):
    """the largest error of the selected rows in units of 2^-8 A (of the bound's floor where A is below it)"""
    return float((np.abs(np.asarray(got, np.float64) - want) / tolerance(A))[sel].max() * MARGIN)


def global_gates_pass(got, want):
    """the two gates of the original test"""
    err = np.abs(np.asarray(got, np.float64) - want)
    return bool(err.max() <= 2e-2 * max(1.0, np.abs(want).max()) and np.sqrt((err ** 2).mean()) <= 3e-3)


# ---------------------------------------------------------------------------------------------------------------- CPU: what the gate rests on
def test_operands_are_exact():
    """The condition the tight gate rests on, for every case of the GPU tests: the operands are exact in bf16, float32 h . w^T + bias in two
    summation orders equals the float64 product, and (the reason: any order) the sum of the products' MAGNITUDES stays below 2^24 units of 2^-8.
    The norm1 cases' LayerNorm rows are on the grid too: exactly gamma z + beta."""
    for c in ALL_CASES:
        ops = c.operands()
        h, w, bias = ops[:3]
        assert np.array_equal(bf16(h), h) and np.array_equal(bf16(w), w), c
        x64 = c.qkv64(h, w, bias)
        b32 = bias if bias is not None else np.zeros(3 * c.D, np.float32)
        one = h @ w.T + b32                                            # the BLAS order, bias last
        two = np.broadcast_to(b32, one.shape).copy()                   # bias first, then slices of 32 k from the last to the first
        for k0 in range(c.D - 32, -1, -32):
            two += h[:, k0:k0 + 32] @ w[:, k0:k0 + 32].T
        assert one.dtype == np.float32 and two.dtype == np.float32
        assert np.array_equal(one.astype(np.float64), x64) and np.array_equal(two.astype(np.float64), x64), c
        assert np.array_equal(np.rint(x64 * 256), x64 * 256), c
        span = float((np.abs(h).astype(np.float64) @ np.abs(w).astype(np.float64).T + np.abs(b32)).max() * 256)
        assert span < 2.0 ** 24, (c, span)
        if c.norm1:
            xres, ln = ops[3:]
            x = xres.reshape(c.B, c.L, c.D)[:, :c.E]
            assert np.isnan(xres.reshape(c.B, c.L, c.D)[:, c.E:]).all()
            mu = np.rint(x.astype(np.float64).mean(-1, keepdims=True))
            assert np.array_equal(h.reshape(c.B, c.L, c.D)[:, :c.E], (x - mu) * ln[0] + ln[1]), c
            assert set(mu.ravel()) == set(MU), c
            # two-pass statistics in float32 give exactly these rows; a one-pass variance is grossly off on the rows of the two large offsets
            x32 = x.astype(np.float32)
            d32 = x32 - x32.mean(-1, keepdims=True, dtype=np.float32)
            two_pass = d32 / np.sqrt((d32 * d32).mean(-1, keepdims=True, dtype=np.float32) + np.float32(1e-5)) * ln[0] + ln[1]
            assert two_pass.dtype == np.float32 and np.array_equal(bf16(two_pass), h.reshape(c.B, c.L, c.D)[:, :c.E]), c
            one_pass = (x32 * x32).mean(-1, dtype=np.float32) - x32.mean(-1, dtype=np.float32) ** 2
            assert (np.abs(one_pass[np.abs(mu[..., 0]) > 4000] - 1) > 0.5).all(), (c, one_pass)


def test_reference_alone_stays_inside_the_gate():
    """emulate_bf16 (the kernel's two roundings and nothing else) of every case passes the gate the kernel is held to; prints the units.
    The largest figure is pinned: above BF16_MARGIN (correct arithmetic cannot meet 1.75 on these cases, which is why MARGIN is the
    analytic 2) and strictly below 2."""
    worst = {}
    for c in ALL_CASES:
        q, k, v = c.qkv_bf16(*c.operands()[:3])
        want, A = reference(q, k, v)
        u = gate(emulate_bf16(q, k, v), want, tolerance(A), f"emulated bf16 arithmetic, {c}") * MARGIN
        print(f"{c}: the two roundings alone: {u:.3f} x 2^-8 A")
        worst[repr(c)] = u
    assert max(worst.values()) <= MARGIN
    assert BF16_MARGIN < worst["D=768 E=2 bias=1 spread=4.0 B=8"] < 1.9, worst
    lo = [u for c, u in zip(ALL_CASES, worst.values()) if c.spread == 1.5]
    hi = [u for c, u in zip(ALL_CASES, worst.values()) if c.spread == 4.0]
    print(f"spread 1.5: {min(lo):.3f} - {max(lo):.3f}; spread 4: {min(hi):.3f} - {max(hi):.3f}")


def test_gates_reject_the_bugs_they_are_meant_to_catch():
    """The per-element gate, applied to float64 references corrupted the way this kernel can go wrong, rejects each of:
      1. the key of extra token 0 (image row 256) left out of the softmax;
      2. two adjacent V rows swapped, at spread 4;
      3. the extra tokens' output rows replaced by those of the second extra token's query (E = 2);
      4. the q bias omitted;
      5. the split chunk's eight partial results merged without the exp(m_w - M) factors (extra-token rows only);
      6. one 32-column weight tile (k1) of one head taken from the next head.
    The exact bf16 rounding of the reference passes.  The two global gates of the original test (max err <= 2e-2 max|out|, rms <= 3e-3) are
    evaluated on the same corrupted references and their verdicts printed: in this gross form (every query of 2 x 8 heads hit, and the worst
    of them decides) they reject these too.  What they cannot see is the small form of the same faults, asserted here:
      7. every extra-token output row off by 1e-2 A (2.56 units) -- the global gates pass it, the per-element gate rejects it;
      8. bug 5 confined to one head of one image."""
    def softmax_v(s, v):
        p = np.exp(s - s.max(-1, keepdims=True))
        return (p @ v) / p.sum(-1, keepdims=True)

    seen = {}
    for spread in (1.5, 4.0):
        c = Case(512, 2, True, spread, 2, seed=11)
        h, w, bias = c.operands()
        E, L, D = c.E, c.L, c.D
        q, k, v = (a.astype(np.float64) for a in c.qkv_bf16(h, w, bias))
        want, A = reference(q, k, v)
        tol = tolerance(A)
        s = q @ k.transpose(0, 1, 3, 2) * 0.125
        good = bf16(want.astype(np.float32))
        assert gate(good, want, tol, "bf16 of the reference") < 1.0 and global_gates_pass(rows(good), rows(want))

        def check(n, bad):
            with pytest.raises(AssertionError):
                gate(bad, want, tol, f"bug {n} at spread {spread}")
            seen[n, spread] = global_gates_pass(rows(bad), rows(want))

        keep = np.arange(L) != 0
        check(1, softmax_v(s[..., keep], v[:, :, keep]))
        vs = v.copy()
        vs[:, :, [E + 10, E + 11]] = v[:, :, [E + 11, E + 10]]
        check(2, softmax_v(s, vs))
        bad = want.copy()
        bad[:, :, 0] = want[:, :, 1]
        check(3, bad)
        nb = bias.copy()
        nb[:D] = 0
        q4 = c.qkv_bf16(h, w, nb)[0].astype(np.float64)
        check(4, softmax_v(q4 @ k.transpose(0, 1, 3, 2) * 0.125, v))
        # the split chunk: wave t holds key tile t of the image rows (token E + r -> row r; tokens 0 .. E - 1 -> rows 256 .., the 9th tile: wave 7)
        tile = np.where(np.arange(L) >= E, (np.arange(L) - E) // 32, 7)
        num, den = 0.0, 0.0
        for t in range(8):
            keys = np.flatnonzero(tile == t)
            st = s[:, :, :E][..., keys]
            pt = np.exp(st - st.max(-1, keepdims=True))
            num, den = num + pt @ v[:, :, keys], den + pt.sum(-1, keepdims=True)
        bad = want.copy()
        bad[:, :, :E] = num / den
        check(5, bad)
        one_head = want.copy()
        one_head[1, 5, :E] = bad[1, 5, :E]
        w6 = w.copy()
        w6[D + 64 * 2 + 32:D + 64 * 3] = w[D + 64 * 3 + 32:D + 64 * 4]
        k6 = c.qkv_bf16(h, w6, bias)[1].astype(np.float64)
        check(6, softmax_v(q @ k6.transpose(0, 1, 3, 2) * 0.125, v))
        bad = want.copy()
        bad[:, :, :E] += 1e-2 * A[:, :, :E]
        check(7, bad)
        check(8, one_head)
    print("the global gates: " + ", ".join(f"bug {n} at spread {sp}: {'PASS' if ok else 'reject'}" for (n, sp), ok in sorted(seen.items())))
    assert seen[7, 1.5] and seen[7, 4.0]


# ---------------------------------------------------------------------------------------------------------------- GPU
def run_rows(c, h, w, bias, xres=None, ln=None):
    """dd_dev_qkv_attention_rows: the whole output buffer [B L + 8, D] of bf16 bits"""
    from duodiff_amd.engine import Context
    ctx = Context.get()
    out = np.full((c.B * c.L + 8, c.D), 0xA5A5, np.uint16)
    h, w = np.ascontiguousarray(h, np.float32), np.ascontiguousarray(w, np.float32)
    ctx.check(ctx.lib.dd_dev_qkv_attention_rows(ctx.handle, c.B, c.L, c.H, c.E, h.ctypes.data, w.ctypes.data, bias.ctypes.data if bias is not None else None,
                                                xres.ctypes.data if xres is not None else None, ln.ctypes.data if ln is not None else None,
                                                out.ctypes.data, 0, None, C.byref(C.c_float(0))))
    return out


def check_output(c, out, want, A, what):
    """canaries, finiteness, the printed units (patch rows | extra-token rows), the per-element gate"""
    body, canary = out[:c.B * c.L], out[c.B * c.L:]
    assert np.all(canary == 0xFFFF), f"{what}: the rows behind the output were written"
    got = from_bf16_bits(body)
    assert np.isfinite(got).all(), f"{what}: a poisoned row reached the output (or a row was not written)"
    ex = c.extra_rows()
    print(f"{what}: max |err| / A = {units(got, want, A, ~ex):.3f} (patch rows) | {units(got, want, A, ex):.3f} (extra-token rows) x 2^-8 (bound {MARGIN})")
    gate(got, want, tolerance(A), what)


def expected(c, h, w, bias):
    want, A = reference(*c.qkv_bf16(h, w, bias))
    return rows(want), rows(A)


@gpu
@pytest.mark.parametrize("c", PER_ELEMENT, ids=repr)
def test_qkv_attention_per_element(c):
    """the hx mode (norm1 rows given): the patch rows of the row-major buffer hold 0xFFFF"""
    h, w, bias = c.operands()
    check_output(c, run_rows(c, h, w, bias), *expected(c, h, w, bias), f"qkv_attention {c}")


@gpu
@pytest.mark.parametrize("c", DOMINANT, ids=repr)
def test_dominant_token_in_every_key_tile(c):
    """One token's row of h doubled (its key then collects the nearly one-hot softmax of the queries it aligns with), in turn in key tiles 0, 1, 3,
    7 and -- tokens 0 and E - 1 -- the 9th: the extra-token queries' maximum then sits in ONE chosen wave of the split chunk, and every other
    wave's partial result has to be scaled down by exp(m_w - M) in the merge.  (Doubling a row doubles its key: it wins where it aligns with
    the query, for 5 - 15 % of the extra-token queries; in the others the maximum sits in whichever wave chance put it -- one, at spread 4.)"""
    h, w, bias = c.operands()
    q, k, v = c.qkv_bf16(h, w, bias)
    s = q[:, :, :c.E].astype(np.float64) @ k.astype(np.float64).transpose(0, 1, 3, 2)
    on_it = s.argmax(-1) == c.doubled
    print(f"{c}: the doubled token holds the largest score of {int(on_it.sum())} of the {on_it.size} extra-token queries")
    assert on_it.any()
    want, A = reference(q, k, v)
    check_output(c, run_rows(c, h, w, bias), rows(want), rows(A), f"qkv_attention {c}")


@gpu
@pytest.mark.parametrize("c", NORM1, ids=repr)
def test_norm1_of_the_extra_rows_in_the_kernel(c):
    """The production mode (hx = nullptr: what Backbone launches): the kernel normalises the extra-token rows itself from the fp32 residual stream.
    Residual rows mu + z with z of mean 0 and variance 1 exactly (+-0.5, +-1, +-2), mu in {0, 100, -2000, 7, 5000, -4097}, gamma in {0.5, 1, 2}, beta a multiple
    of 0.25 that cancels no gamma z (so |gamma z + beta| >= 0.25 where |gamma z| <= 4): norm1 is within 5e-6 |gamma z| (the eps), at most 4e-5
    relative, of a value of at most 5 significant bits, whose nearest bf16 rounding boundary is 2^-9 = 2e-3 relative away -- 50 times further,
    and 10^4 times further than fp32 arithmetic moves it -- so bf16(float64 LayerNorm) is what a correct kernel holds -- (a) bit-identical to the hx-mode run given those rows,
    (b) inside the per-element gate against float64, (c) finite although the patch rows of xres hold NaN.  A one-pass variance in fp32 is 0 or 2
    instead of 1 on the 5000 and -4097 rows (MU above): a kernel built that way missed the gate of all six cases by a factor of 10^6."""
    h, w, bias, xres, ln = c.operands()
    want, A = expected(c, h, w, bias)
    given = run_rows(c, h, w, bias)
    hp = h.copy()
    hp.reshape(c.B, c.L, c.D)[:, :c.E] = np.nan          # (ignored in this mode)
    own = run_rows(c, hp, w, bias, xres, ln)
    check_output(c, given, want, A, f"qkv_attention hx mode {c}")
    check_output(c, own, want, A, f"qkv_attention production mode {c}")
    differ = np.argwhere(own != given)
    assert differ.size == 0, f"{c}: {len(differ)} elements differ between the two modes, first at {differ[0]}"


@gpu
@pytest.mark.parametrize("D,E", [(512, 2), (768, 1)])
def test_an_image_does_not_depend_on_its_batch_or_its_workgroup_map(D, E):
    """images 0 .. 2 of a B = 8 run (XCD-grouped map) are bit-equal to the B = 3 run of those images (plain map); images 8 .. 12 of a B = 16 run
    (the second group of 8: b = (blockIdx & 7) + 8 (slot / H)) to a B = 5 run of those"""
    for B, first, n in ((8, 0, 3), (16, 8, 5)):
        c = Case(D, E, True, 1.5, B, seed=D + B)
        h, w, bias = c.operands()
        whole = run_rows(c, h, w, bias)
        sub = Case(D, E, True, 1.5, n, seed=0)
        part = run_rows(sub, h[first * c.L:(first + n) * c.L], w, bias)
        assert np.isfinite(from_bf16_bits(whole[:B * c.L])).all()
        assert np.array_equal(whole[first * c.L:(first + n) * c.L], part[:n * c.L]), (D, E, B)


@gpu
def test_refused_shapes_write_nothing():
    """extras = 3, extras = 0, L != 256 + extras and H = 4 (D = 256), in both modes: DD_ERR_UNSUPPORTED, the caller's out buffer as it was"""
    from duodiff_amd import _lib
    from duodiff_amd.engine import Context
    ctx = Context.get()
    for B, L, H, extras in [(2, 259, 8, 3), (2, 256, 8, 0), (2, 257, 8, 2), (2, 258, 12, 1), (2, 257, 4, 1)]:
        D = 64 * H
        z = np.zeros((B * L, D), np.float32)
        w, ln = np.zeros((3 * D, D), np.float32), np.ones((2, D), np.float32)
        for xres in (None, z):
            out = np.full((B * L + 8, D), 0xA5A5, np.uint16)
            st = ctx.lib.dd_dev_qkv_attention_rows(ctx.handle, B, L, H, extras, z.ctypes.data, w.ctypes.data, None,
                                                   xres.ctypes.data if xres is not None else None, ln.ctypes.data if xres is not None else None,
                                                   out.ctypes.data, 0, None, C.byref(C.c_float(0)))
            assert st == _lib.DD_ERR_UNSUPPORTED, (B, L, H, extras, st)
            assert np.all(out == 0xA5A5), (B, L, H, extras)
