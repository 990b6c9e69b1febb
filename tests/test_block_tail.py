"""GPU unit tests of the block tail as the model launches it (csrc/mlp_fused.hip: mlp_fused_kernel, mlp_reduce_kernel, skip_rows_ln_kernel,
qkv_rows_kernel) through the development entry point dd_dev_block_tail (include/duodiff_dev.h), which fills MlpFusedArgs and runs the launch
sequence of Backbone::block_tail: B images of n_patches patch tokens behind `extras` extra tokens, every mode of the model (projection in front,
norm1 row-major or in fragment order, skip_linear, the y tap of early-exit models, attn.qkv, the last block's launch).

Operands whose roundings are known bit for bit (the method of tests/test_qkv_attention.py).  The tail rounds to bf16 at two points that are never
stored -- norm2's output and the hidden activation -- so the rows are built such that norm2 is exact: x1 = mu + s0 z with z a permutation of
{+-0.5 x 5D/8, +-1.5 x 3D/8} (mean 0, variance 1 exactly), gamma in +-{0.5, 1, 2}, beta an odd multiple of 1/8: norm2(x1) = z gamma + beta up to the
1e-5 eps, every value on a 2^-3 grid and at least 8 x further from a bf16 rounding boundary than the eps moves it.  With the projection in front,
ao, Wproj and bproj lie on a 2^-3 grid and x = x1 - (ao Wproj^T + bproj) is exact in fp32, so fp32 accumulation gives x1 exactly, in any order.
test_operands_are_exact (CPU) asserts all of that for every operand set.  fc1 is dense with b1 a permutation of linspace(-12, 12): the
pre-activations cover the GELU polynomial, its +-3.8 clamp and both tails.  fc2 is sparse -- output column j sums hidden / D hidden units
sigma(4 j + i) with weights +-2^-e -- so that every hidden unit (every chunk, every accumulator slot) is seen through exactly one output element
and the bound is sharp; one dense-W2 case per mode family keeps the aggregate gates of tests/test_mlp_fused.py.

Gates, all elementwise (gate() of tests/kernel_support.py), s = the float64 pre-activation of the exact operands:
  * hidden activation   Eg = ulp_bf16(gelu(s)) + GELU_POLY + GELU_SLOPE FP32_REL (|h2| |W1|^T + |b1|)
  * y (xres; y_tap)     |got - ref| <= Eg |W2|^T + FP32_REL (|gelu(s)| |W2|^T + |b2| + |x1|)        (the reference leaves the activation unrounded)
  * bf16 copy           bit-equal to bf16() of the fp32 rows that came back
  * norm1               ln_ref_and_tol of the kernel's own fp32 rows, row-major and unfrag(ln_out_frag)
  * skip_linear + tap   [bf16(y_tap) | bf16(skip)] bf16(Wskip)^T + bskip from the kernel's OWN y_tap, bound FP32_REL (|cat| |Wskip|^T + |bskip|): the
                        SKIP phases' B operand is cvt_pk_bf16 of exactly the value the tap stores (mlp_body: `q += b2; tap = q; u = cvt_pk_bf16(q)`),
                        the extra-token rows' y travels through the bf16 copy (mlp_reduce_kernel stores f2bf of the value it taps)
  * skip_linear, no tap the reference is built from the float64 y, with one bf16 ulp of y times |Wskip_y|^T added to the bound (the kernel rounds ITS y);
                        the extra-token rows' y is taken from the bf16 copy in either mode, and that copy, where no fp32 y comes back, is gated
                        against the float64 y with Ey + one ulp (the rounding of a value within Ey of the reference)
  * attn.qkv            the gate of test_mlp_fused.py::test_fused_tail_with_next_qkv, unchanged
Every buffer comes back whole: rows >= M, the fragment buffer past its last 32-row group, the slab area past tiles_left x groups x prows x D, the
rows [L, Lp) of the head-major image and the space behind it must still hold 0xFF; the rows [M, Mo) of every operand and the slab buffer hold NaN
on the device.  Contract notes read from the code: a SKIP launch writes the bf16 copy for the extra-token rows only (the main tiles keep y in
registers); a QKV launch writes norm1 for the extra-token rows only, and its stores of rows past a ragged tile go to MlpFusedArgs::qkv_dump, a
16 KB scratch of the launch that is no output; in fragment-order mode nothing is written to the row-major norm1 buffer.
"""
import ctypes as C
import functools
import re
from pathlib import Path

import numpy as np
import pytest

from duodiff_amd._lib import DD_ERR_UNSUPPORTED
from kernel_support import (FP32_REL, GELU_POLY, GELU_SLOPE, NAN16, NAN32, P, bf16, bf16_bits, from_bf16_bits, gate, gelu_exact, ln_ref_and_tol,
                            round_up, to_frag, unfrag, untouched, ulp_bf16)
from oracle.uvit_oracle import layer_norm

gpu = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]


# ---------------------------------------------------------------------------------------------------------------- the kernel's GELU polynomial
@functools.lru_cache(None)
def gelu_literals():
    """the coefficients of the DD_S_G* statements of mlp_fused.hip as floats, highest power first (halved: 0.5 erf(s / sqrt2) / s), and the clamp"""
    src = (REPO / "duodiff_amd" / "csrc" / "mlp_fused.hip").read_text()
    hexes = []
    for line in src.splitlines():
        if line.startswith("#define DD_S_G"):
            for hx in re.findall(r"0x[0-9a-fA-F]{8}", line):
                if hx not in hexes:
                    hexes.append(hx)
    lit = [np.array([int(hx, 16)], np.uint32).view(np.float32)[0] for hx in hexes]
    m = re.search(r"const GeluConst gk\{([0-9.]+)f, 0\.5f \* (-?[0-9.e+-]+)f\}", src)
    hi, c5 = np.float32(m.group(1)), np.float32(0.5) * np.float32(m.group(2))
    assert len(lit) == 7 and lit[-1] == np.float32(0.5), hexes
    return [lit[0], c5] + lit[1:6], hi      # c6, c5, c4 .. c0; the trailing 0.5 is the constant term of 0.5 + s P'(s^2)


def gelu_poly(v, clamp=True):
    """the kernel's GELU in fp32: v (0.5 + s P'(s^2)), s = med3(v, +-3.8)"""
    coef, hi = gelu_literals()
    v = np.asarray(v, np.float32)
    sc = np.clip(v, -hi, hi) if clamp else v
    s2 = sc * sc
    p = s2 * coef[0] + coef[1]
    for c in coef[2:]:
        p = (p * s2 + c).astype(np.float32)
    h = (sc * p + np.float32(0.5)).astype(np.float32)
    return (h * v).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- operands
MODES = {          # name -> the set of switches (x: h given, no LayerNorm prologue; n1: norm1 out, row-major)
    "plain": {"x"}, "ln": set(), "proj+n1": {"proj", "n1"}, "proj+frag": {"proj", "frag"}, "proj+skip+n1": {"proj", "skip", "n1"},
    "proj+skip+frag": {"proj", "skip", "frag"}, "proj+skip+tap": {"proj", "skip", "tap"}, "proj+skip+tap+frag": {"proj", "skip", "tap", "frag"},
    "proj+qkv": {"proj", "qkv"}, "proj+skip+qkv": {"proj", "skip", "qkv"}, "last": {"proj", "last"}, "proj": {"proj"},
}


class Ops:
    """one operand set: B images of N patch tokens behind E extra tokens, width D; every array as the kernel sees it (bf16 operands are
    already bf16-exact), and the float64 model of the tail built from them (ref())"""

    def __init__(self, B, N, E, D, dense=False, seed=0):
        self.B, self.N, self.E, self.D, self.dense = B, N, E, D, dense
        self.L, self.M, self.hidden = N + E, B * (N + E), 4 * D
        M, hidden = self.M, self.hidden
        r = np.random.default_rng([B, N, E, D, int(dense), seed])
        base = np.concatenate([np.full(5 * D // 16, 0.5), np.full(5 * D // 16, -0.5), np.full(3 * D // 16, 1.5), np.full(3 * D // 16, -1.5)])
        self.z = r.permuted(np.tile(base, (M, 1)), axis=1)
        self.s0 = r.choice([0.5, 1.0, 2.0], (M, 1))
        self.mu = r.integers(-16, 17, (M, 1)) * 0.25
        x1 = self.mu + self.s0 * self.z
        self.gamma = r.choice([0.5, 1.0, 2.0], D) * r.choice([-1.0, 1.0], D)
        self.beta = (2 * r.integers(-4, 4, D) + 1) / 8.0
        self.h2 = self.z * self.gamma + self.beta                      # norm2(x1) as the kernel rounds it: exact in bf16
        self.ao = r.integers(-16, 17, (M, D)) / 8.0
        self.wproj = r.integers(-8, 9, (D, D)) / 8.0
        self.bproj = r.integers(-16, 17, D) / 8.0
        x0 = x1 - (self.ao @ self.wproj.T + self.bproj)                # float64, exact
        self.x1_64, self.x0_64 = x1, x0
        self.x1, self.x0 = x1.astype(np.float32), x0.astype(np.float32)
        self.w1 = bf16((0.4 / np.sqrt(D)) * r.standard_normal((hidden, D)))
        self.b1 = r.permutation(np.linspace(-12, 12, hidden)).astype(np.float32)
        sigma = r.permutation(hidden).reshape(D, hidden // D)
        w2 = np.zeros((D, hidden), np.float32)
        w2[np.arange(D)[:, None], sigma] = r.choice([-1.0, 1.0], sigma.shape) * 2.0 ** -r.integers(0, 3, sigma.shape)
        self.sigma = sigma
        self.w2 = bf16(0.05 * r.standard_normal((hidden, D)).T) if dense else w2
        self.b2 = (0.2 * r.standard_normal(D)).astype(np.float32)
        self.ln_out = ((1.0 + 0.3 * r.standard_normal(D)).astype(np.float32), (0.2 * r.standard_normal(D)).astype(np.float32))
        self.skip = bf16(1.2 * r.standard_normal((M, D)))
        self.wskip = bf16(0.04 * r.standard_normal((D, 2 * D)))
        self.bskip = (0.2 * r.standard_normal(D)).astype(np.float32)
        self.wqkv = bf16(0.05 * r.standard_normal((3 * D, D)))
        self.patch = (np.arange(M) % self.L) >= E
        self._ref = None

    def image(self, b):
        """the operand set of image b alone (B = 1): the same weights, its rows"""
        o = Ops.__new__(Ops)
        o.__dict__.update(self.__dict__)
        o.B, o.M, o._ref = 1, self.L, None
        rows = slice(b * self.L, (b + 1) * self.L)
        for k in ("z", "s0", "mu", "h2", "ao", "x1_64", "x0_64", "x1", "x0", "skip", "patch"):
            setattr(o, k, np.ascontiguousarray(getattr(self, k)[rows]))
        return o

    def ref(self):
        """float64: s, g = gelu(s) (unrounded), y, and the elementwise bounds Eg, Ey"""
        if self._ref is None:
            w1, w2 = self.w1.astype(np.float64), self.w2.astype(np.float64)
            s = self.h2 @ w1.T + self.b1
            g = gelu_exact(s)
            Eg = ulp_bf16(g) + GELU_POLY + GELU_SLOPE * FP32_REL * (np.abs(self.h2) @ np.abs(w1).T + np.abs(self.b1))
            gg = bf16(g.astype(np.float32)).astype(np.float64) if self.dense else g      # (dense: the reference of test_mlp_fused.py)
            y = self.x1_64 + gg @ w2.T + self.b2
            Ey = Eg @ np.abs(w2).T + FP32_REL * (np.abs(g) @ np.abs(w2).T + np.abs(self.b2) + np.abs(self.x1_64))
            self._ref = dict(s=s, g=g, Eg=Eg, y=y, Ey=Ey)
        return self._ref


@functools.lru_cache(None)
def ops_for(B, N, E, D, dense=False):
    return Ops(B, N, E, D, dense)


def slab_rows_for(o, sw):
    tiles_left = 0 if "last" in sw else (o.B * o.E + 31) // 32
    return tiles_left * 16 * 32 + 8


# ---------------------------------------------------------------------------------------------------------------- the GPU call
def run(o, mode, poison=0xFF):
    """dd_dev_block_tail; every buffer whole.  poison: the byte the padding rows of the operands (xres included) and the slab buffer hold"""
    from duodiff_amd.engine import Context
    ctx = Context.get()
    sw = MODES[mode]
    M, D = o.M, o.D
    Mo = round_up(M, 256) + 8
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    proj, skp, qk = "proj" in sw, "skip" in sw, "qkv" in sw
    lnout = bool(sw & {"n1", "frag", "skip", "qkv"})
    xres = np.full((Mo, D), poison * 0x01010101, np.uint32).view(np.float32)
    xres[:M] = o.x0 if proj else o.x1
    res = dict(xres=xres, M=M, Mo=Mo, mode=mode, poison=poison)
    res["out"] = None if "last" in sw else np.zeros((Mo, D), np.uint16)
    res["ln"] = np.zeros((Mo, D), np.uint16) if lnout else None
    res["frag"] = np.zeros(Mo * D, np.uint16) if "frag" in sw else None
    res["tap"] = np.zeros((Mo, D), np.float32) if "tap" in sw else None
    H, Lp = D // 64, round_up(o.L, 8)
    res["qkv"] = np.zeros((o.B * 3 * H * Lp + 64) * 64, np.uint16) if qk else None
    srows = slab_rows_for(o, sw)
    res["slab"] = np.zeros((srows, D), np.float32)
    plan = (C.c_int * 4)()
    keep = [f32(o.h2) if "x" in sw else None, f32(o.w1), f32(o.b1), f32(o.w2), f32(o.b2),
            None if "x" in sw else f32(np.stack([o.gamma, o.beta])),
            f32(o.ao) if proj else None, f32(o.wproj) if proj else None, f32(o.bproj) if proj else None,
            f32(np.stack(o.ln_out)) if lnout else None,
            f32(o.skip) if skp else None, f32(o.wskip) if skp else None, f32(o.bskip) if skp else None, f32(o.wqkv) if qk else None]
    st = ctx.lib.dd_dev_block_tail(ctx.handle, o.B, o.N, o.E, D, o.hidden, 1 if "last" in sw else 0, poison, *[P(a) for a in keep],
                                   P(xres), P(res["out"]), P(res["ln"]), P(res["frag"]), P(res["tap"]), P(res["qkv"]), P(res["slab"]), srows,
                                   C.cast(plan, C.c_void_p), 0, None, C.byref(C.c_float(0)))
    res["status"] = st
    if st == DD_ERR_UNSUPPORTED:
        return res
    ctx.check(st)
    res["plan"] = tuple(plan)
    return res


# ---------------------------------------------------------------------------------------------------------------- the kernel emulated on the CPU
def emulate(o, mode, bug=None):
    """what a correct kernel returns, from the float64 model with the kernel's roundings applied to it (fp32 pre-activation, the kernel's polynomial,
    bf16 activation, fp32 rows, bf16 copies), in the buffers of run() with their canaries -- or one of the bugs the gates are meant to catch"""
    sw = MODES[mode]
    M, D, E, L, hidden = o.M, o.D, o.E, o.L, o.hidden
    Mo = round_up(M, 256) + 8
    ref = o.ref()
    b1 = o.b1.astype(np.float64).copy()
    if bug == "b1p":                  # two hidden units of one chunk (its largest and its smallest bias) exchange their slots in the accumulator-order table
        u0, u1 = 32 * 5 + int(np.argmax(b1[160:192])), 32 * 5 + int(np.argmin(b1[160:192]))
        b1[[u0, u1]] = b1[[u1, u0]]
    s32 = (o.h2 @ o.w1.astype(np.float64).T + b1).astype(np.float32)
    p = bf16(gelu_poly(s32, clamp=bug != "noclamp")).astype(np.float64)
    if bug == "chunk":                # rows 32 .. 63 (one wave of the first main tile) without hidden units 96 .. 127
        rows = np.flatnonzero(o.patch)[32:64]
        p[rows[:, None], np.arange(96, 128)] = 0.0
    y = (o.x1_64 + p @ o.w2.astype(np.float64).T + o.b2).astype(np.float32)
    if bug == "tok_e":                # patch rows read at b tok_l + p, without + tok_e: row r computes from the operands of row r - E
        y2 = y.copy()
        y2[o.patch] = y[np.flatnonzero(o.patch) - E]
        y = y2
    if bug == "tok_l":                # the image of a patch row taken with tok_l = N: image b's patch rows computed from the rows b E further up
        y2 = y.copy()
        y2[o.patch] = y[np.flatnonzero(o.patch) - E * (np.flatnonzero(o.patch) // L)]
        y = y2
    if bug == "ragged":               # the last, ragged 32-row group of every image left out: its rows keep what the launch found in x
        rows = np.flatnonzero(o.patch & ((np.arange(M) % L) - E >= o.N // 32 * 32))
        y = y.copy()
        y[rows] = (o.x0 if "proj" in sw else o.x1)[rows]
    res = dict(M=M, Mo=Mo, mode=mode, poison=0xFF, status=0)
    full32 = lambda rows_: np.concatenate([rows_, np.full((Mo - M, D), NAN32, np.uint32).view(np.float32)])
    blank16 = lambda: np.full((Mo, D), NAN16, np.uint16)
    xrows = y
    out = blank16()
    if "skip" in sw:
        out[:M][~o.patch] = bf16_bits(y[~o.patch])
        cat = np.concatenate([bf16(y), o.skip], axis=1).astype(np.float64)
        xrows = (cat @ o.wskip.astype(np.float64).T + o.bskip).astype(np.float32)
        res["tap"] = full32(y) if "tap" in sw else None
    else:
        out[:M] = bf16_bits(y)
        res["tap"] = None
    if "last" in sw:
        xrows = xrows.copy()
        xrows[~o.patch] = o.x0[~o.patch]
        out = None
    res["xres"], res["out"] = full32(xrows), out
    lnout = bool(sw & {"n1", "frag", "skip", "qkv"})
    res["ln"] = res["frag"] = res["qkv"] = None
    n_main = int(o.patch.sum())
    if lnout:
        h = bf16_bits(layer_norm(xrows, *o.ln_out))
        ln = blank16()
        if "frag" in sw:
            fr = np.full(Mo * D, NAN16, np.uint16)
            fr[: n_main * D] = to_frag(h[o.patch], D, swap_halves=bug == "halves")
            res["frag"] = fr
        elif "qkv" in sw:
            ln[:M][~o.patch] = h[~o.patch]
        else:
            ln[:M] = h
        res["ln"] = ln
        if "qkv" in sw:
            H, Lp = D // 64, round_up(L, 8)
            q = bf16_bits((from_bf16_bits(h).astype(np.float64) @ o.wqkv.astype(np.float64).T).astype(np.float32))      # [M, 3 D]
            img = np.full((o.B, 3 * H, Lp, 64), NAN16, np.uint16)
            img[:, :, :L, :] = q.reshape(o.B, L, 3 * H, 64).transpose(0, 2, 1, 3)
            res["qkv"] = np.concatenate([img.reshape(-1), np.full(64 * 64, NAN16, np.uint16)])
    tiles_left = 0 if "last" in sw else (o.B * E + 31) // 32
    groups = min(hidden // 64, 16)
    res["plan"] = ((n_main + 127) // 128, tiles_left, groups, 32)
    slab = np.full((slab_rows_for(o, sw), D), NAN32, np.uint32).view(np.float32)
    slab[: tiles_left * groups * 32] = 0.0
    res["slab"] = slab
    return res


# ---------------------------------------------------------------------------------------------------------------- the gates
def check(o, res):
    """every gate and canary of the module docstring on the buffers of one launch; returns {gate: {row class: largest error / bound}}"""
    sw = MODES[res["mode"]]
    M, D, E, L, B = o.M, o.D, o.E, o.L, o.B
    ref = o.ref()
    patch = o.patch
    classes = {"patch": patch, "extra": ~patch}
    name = f"{res['mode']} B={B} N={o.N} E={E} D={D}{' dense' if o.dense else ''}"
    xres, out, ln, fr, tap, qkv, slab = (res[k] for k in ("xres", "out", "ln", "frag", "tap", "qkv", "slab"))
    ratios = {}
    x = xres[:M]
    last = "last" in sw
    skp = "skip" in sw

    def gate_y(got, rows, what):
        if o.dense:      # the aggregate gates of tests/test_mlp_fused.py: dense rounding noise through K = hidden has no useful worst-case bound
            err = np.abs(got[rows].astype(np.float64) - ref["y"][rows])
            scale = max(float(np.abs(ref["y"] - o.x1_64).std()), 0.1)
            assert np.isfinite(got[rows]).all(), f"{name}: {what}: not finite"
            assert err.max() <= 1.5e-2 * scale and np.sqrt((err ** 2).mean()) <= 2e-3 * scale, f"{name}: {what}: max {err.max():.3e} rms {np.sqrt((err ** 2).mean()):.3e}"
            return float(err.max() / (1.5e-2 * scale))
        return gate(got[rows], ref["y"][rows], ref["Ey"][rows], f"{name}: {what}")

    # ---- y: xres without skip_linear, y_tap with the tap
    ysrc = tap[:M] if tap is not None else (None if skp else x)
    if ysrc is not None:
        ratios["y"] = {c: gate_y(ysrc, rows, f"y ({c} rows)") for c, rows in classes.items() if rows.any() and not (last and c == "extra")}
    if last:
        assert np.array_equal(x[~patch].view(np.uint32), o.x0[~patch].view(np.uint32)), f"{name}: the last block's launch wrote extra-token rows of x"
    # ---- the bf16 copy
    if out is not None:
        if skp:      # the extra-token rows only: y on its way to skip_rows_ln_kernel
            assert untouched(out[:M][patch]), f"{name}: a SKIP launch wrote the bf16 copy of patch rows"
            if tap is not None:
                assert np.array_equal(out[:M][~patch], bf16_bits(tap[:M][~patch])), f"{name}: bf16 copy != bf16(y_tap) on the extra-token rows"
            elif E and not o.dense:
                r_ = ~patch
                ratios["copy"] = {"extra": gate(from_bf16_bits(out[:M][r_]), ref["y"][r_], ref["Ey"][r_] + ulp_bf16(ref["y"][r_]), f"{name}: bf16 copy of y")}
        else:
            rows = patch if last else np.ones(M, bool)
            assert np.array_equal(out[:M][rows], bf16_bits(x[rows])), f"{name}: bf16 copy != bf16 of the fp32 rows"
            assert untouched(out[:M][~rows]), f"{name}: bf16 copy of rows the launch does not compute"
        assert untouched(out[M:]), f"{name}: bf16 copy rows >= M written"
    # ---- skip_linear
    if skp:
        wsk = o.wskip.astype(np.float64)
        ycat = np.empty((M, D), np.float32)
        extra_tol = np.zeros((M, D))
        if tap is not None:
            ycat[patch] = bf16(tap[:M][patch])
        else:
            ycat[patch] = bf16(ref["y"][patch].astype(np.float32))
            extra_tol[patch] = ulp_bf16(ref["y"][patch]) @ np.abs(wsk[:, :D]).T
        ycat[~patch] = from_bf16_bits(out[:M][~patch])      # the extra-token rows' y travels through the bf16 copy
        cat = np.concatenate([ycat, o.skip], axis=1).astype(np.float64)
        want = cat @ wsk.T + o.bskip
        tol = FP32_REL * (np.abs(cat) @ np.abs(wsk).T + np.abs(o.bskip)) + extra_tol
        if o.dense and tap is None:      # the aggregate gate of test_fused_tail_with_next_skip_linear
            err = np.abs(x[patch] - want[patch])
            scale = max(float(want.std()), 0.1)
            assert err.max() <= 3e-2 * scale and np.sqrt((err ** 2).mean()) <= 4e-3 * scale, f"{name}: x' max {err.max():.3e}"
            ratios["skip"] = {"patch": float(err.max() / (3e-2 * scale)), "extra": gate(x[~patch], want[~patch], tol[~patch], f"{name}: x' (extra rows)")}
        else:
            ratios["skip"] = {c: gate(x[rows], want[rows], tol[rows], f"{name}: x' = skip_linear ({c} rows)") for c, rows in classes.items() if rows.any()}
    assert untouched(xres[M:]) if res["poison"] == 0xFF else bool(np.all(xres[M:].view(np.uint8) == res["poison"])), f"{name}: x rows >= M written"
    assert np.isfinite(x).all(), f"{name}: x is not finite"
    if tap is not None:
        assert untouched(tap[M:]), f"{name}: y_tap rows >= M written"
        assert np.isfinite(tap[:M]).all(), f"{name}: y_tap is not finite"
    # ---- norm1 of the kernel's own rows: row-major, fragment order
    n_main = int(patch.sum())
    if ln is not None:
        want, tol = ln_ref_and_tol(x, *o.ln_out)
        if fr is not None:
            assert untouched(ln), f"{name}: fragment-order mode wrote the row-major norm1 buffer"
            got = from_bf16_bits(unfrag(fr, n_main // 32, D))
            ratios["norm1 frag"] = {"patch": gate(got, want[patch], tol[patch], f"{name}: norm1 (fragment order)")}
            assert untouched(fr[n_main * D:]), f"{name}: fragment buffer written past its last 32-row group"
        else:
            rows = ~patch if qkv is not None else np.ones(M, bool)
            ratios["norm1"] = {c: gate(from_bf16_bits(ln[:M][r_ & rows]), want[r_ & rows], tol[r_ & rows], f"{name}: norm1 ({c} rows)")
                               for c, r_ in classes.items() if (r_ & rows).any()}
            assert untouched(ln[:M][~rows]), f"{name}: a QKV launch wrote norm1 of patch rows"
            assert untouched(ln[M:]), f"{name}: norm1 rows >= M written"
    # ---- attn.qkv: the gate of test_mlp_fused.py::test_fused_tail_with_next_qkv
    if qkv is not None:
        H, Lp = D // 64, round_up(L, 8)
        img = qkv[: B * 3 * H * Lp * 64].reshape(B, 3 * H, Lp, 64)
        x64 = x.astype(np.float64)
        mu = x64.mean(-1, keepdims=True)
        hn = ((x64 - mu) / np.sqrt(((x64 - mu) ** 2).mean(-1, keepdims=True) + 1e-5) * o.ln_out[0] + o.ln_out[1]).astype(np.float32)
        want = bf16(hn).astype(np.float64) @ o.wqkv.astype(np.float64).T
        have = from_bf16_bits(img[:, :, :L, :]).transpose(0, 2, 1, 3).reshape(M, 3 * D)
        err = np.abs(have - want)
        scale = max(float(want.std()), 0.1)
        assert np.isfinite(have).all(), f"{name}: qkv is not finite"
        assert err.max() <= 2.5e-2 * scale and np.sqrt((err ** 2).mean()) <= 3e-3 * scale, f"{name}: qkv max {err.max():.3e} rms {np.sqrt((err ** 2).mean()):.3e}"
        ratios["qkv"] = {c: float(err[rows].max() / (2.5e-2 * scale)) for c, rows in classes.items() if rows.any()}
        assert untouched(img[:, :, L:, :]), f"{name}: rows [L, Lp) of the head-major image written"
        assert untouched(qkv[B * 3 * H * Lp * 64:]), f"{name}: bytes behind the head-major image written"
    # ---- the slabs
    tiles_main, tiles_left, groups, prows = res["plan"]
    assert tiles_main == (n_main + 127) // 128 and tiles_left == (0 if last else (B * E + 31) // 32), f"{name}: plan {res['plan']}"
    used = tiles_left * groups * prows
    assert np.isfinite(slab[:used]).all(), f"{name}: a slab row inside the plan is not finite"
    assert bool(np.all(slab[used:].view(np.uint8) == res["poison"])), f"{name}: slab area past tiles_left x groups x prows x D written"
    print(f"{name}: max err/bound " + "; ".join(f"{k} " + ", ".join(f"{c} {v:.3f}" for c, v in d.items()) for k, d in ratios.items()))
    return ratios


def same_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ---------------------------------------------------------------------------------------------------------------- cases
G17 = (17, 32, 2)        # 544 patch rows: four main tiles + a ragged fifth of 32 rows, tiles straddle four images; 34 extra rows: a 2nd hidden-split tile of 2
GEOMETRIES = [(1, 256, 1), (3, 256, 2), G17, (3, 96, 1), (1, 300, 0)]
CASES = ([(G17, 512, m, False) for m in ("plain", "ln", "proj+n1", "proj+frag", "proj+skip+n1", "proj+skip+frag", "proj+skip+tap", "proj+qkv",
                                        "proj+skip+qkv", "last")]
         + [(g, 512, m, False) for g in GEOMETRIES if g != G17 for m in ("proj+frag", "proj+skip+tap") if not (m == "proj+frag" and g[1] % 32)]
         + [(G17, d, m, False) for d in (128, 256) for m in ("ln", "proj+frag", "proj+skip+n1", "proj+skip+tap", "proj+skip+qkv")]
         + [(G17, 64, "ln", False), (G17, 64, "plain", False), ((1, 300, 0), 512, "plain", False), ((1, 300, 0), 512, "proj+n1", False)]
         + [(G17, 512, m, True) for m in ("plain", "proj+n1", "proj+skip+n1", "proj+skip+tap")])
OPERAND_SETS = sorted({(g, d, dense) for g, d, _, dense in CASES})


def case_id(c):
    (B, N, E), D, m, dense = c
    return f"B{B}-N{N}-E{E}-D{D}-{m}{'-dense' if dense else ''}"


# ---------------------------------------------------------------------------------------------------------------- CPU tests
@pytest.mark.parametrize("geom,D,dense", OPERAND_SETS, ids=lambda v: str(v).replace(" ", ""))
def test_operands_are_exact(geom, D, dense):
    """x, x1 and the grid products are exact in fp32, and a float32 LayerNorm written two ways -- two-pass, and shifted one-pass over the two lane
    halves' columns as ln_stats_shifted -- rounds to the target bits; the pre-activations stay inside the range the GELU bound is stated for"""
    o = ops_for(*geom, D, dense)
    f = np.float32
    assert np.array_equal(o.x1.astype(np.float64), o.x1_64) and np.array_equal(o.x0.astype(np.float64), o.x0_64)
    for a in (o.ao, o.wproj, o.bproj, o.h2, o.gamma, o.beta):
        assert np.array_equal(bf16(a.astype(f)).astype(np.float64), a)            # exact bf16 operands / targets
    assert np.all(np.abs(o.h2) >= 0.125) and np.all(o.h2 * 8 == np.round(o.h2 * 8))
    # fp32 accumulation, k ascending from x + bproj as the kernel's accumulators do, and as one fp32 matmul: x1 exactly
    acc = (o.x0 + o.bproj.astype(f)).astype(f)
    aof, wpf = o.ao.astype(f), o.wproj.astype(f)
    for k0 in range(0, D, 16):
        acc = (acc + aof[:, k0:k0 + 16] @ wpf[:, k0:k0 + 16].T).astype(f)
    assert np.array_equal(acc, o.x1)
    assert np.array_equal(((aof @ wpf.T) + o.bproj.astype(f) + o.x0).astype(f), o.x1)
    # LayerNorm in fp32, two ways
    x, g, b = o.x1, o.gamma.astype(f), o.beta.astype(f)
    target = bf16_bits(o.h2)
    mean = x.mean(-1, keepdims=True, dtype=f)
    var = ((x - mean) ** 2).mean(-1, keepdims=True, dtype=f)
    two = ((x - mean) * (f(1) / np.sqrt(var + f(1e-5))) * g + b).astype(f)
    assert np.array_equal(bf16_bits(two), target)
    half = (np.arange(D) % 8) // 4                                                 # lane half h holds columns 8 g + 4 h .. + 3
    n = f(D // 2)
    mh, m2h = [], []
    for h in (0, 1):
        xh = x[:, half == h]
        c = xh[:, :1]
        d = (xh - c).astype(f)
        s, q = d.sum(-1, keepdims=True, dtype=f), (d * d).sum(-1, keepdims=True, dtype=f)
        mh.append((c + s / n).astype(f))
        m2h.append((q - s * s / n).astype(f))
    mean1 = (f(0.5) * (mh[0] + mh[1])).astype(f)
    dd = (mh[0] - mh[1]).astype(f)
    var1 = (((m2h[0] + m2h[1]) + dd * dd * (f(0.5) * n)) / f(D)).astype(f)
    rstd = (f(1) / np.sqrt(np.maximum(var1, f(0)) + f(1e-5))).astype(f)
    one = ((x * rstd + (-mean1 * rstd)) * g + b).astype(f)
    assert np.array_equal(bf16_bits(one), target)
    dev = max(float(np.abs(two - o.h2).max()), float(np.abs(one - o.h2).max()))
    assert dev <= 1e-4, dev                                                        # against a smallest half-ulp of 2^-11 = 4.9e-4
    # sparse fc2: every hidden unit is seen through exactly one output element
    if not dense:
        assert np.array_equal(np.sort(o.sigma.reshape(-1)), np.arange(o.hidden)) and np.all((o.w2 != 0).sum(0) == 1)
        assert np.all((o.w2 != 0).sum(1) == o.hidden // D)
    assert float(np.abs(o.ref()["s"]).max()) <= 16.0


def test_gates_reject_the_bugs_they_are_meant_to_catch():
    """check() applied to the float64 model of the tail with the kernel's roundings emulated on it (emulate()): a correct kernel passes every gate
    with a ratio below 1, each of five bugs is rejected, and the kernel's GELU polynomial stays within GELU_POLY of the exact GELU"""
    o = ops_for(3, 32, 2, 128)
    worst = {}
    for mode in ("ln", "plain", "proj+n1", "proj+frag", "proj+skip+n1", "proj+skip+frag", "proj+skip+tap", "proj+qkv", "proj+skip+qkv", "last"):
        for k, d in check(o, emulate(o, mode)).items():
            worst[k] = max(worst.get(k, 0.0), max(d.values()))
    print("the reference's own roundings, largest error / bound:", worst)
    assert all(v < 1.0 for v in worst.values()), worst
    # the five bugs
    for bug, mode in (("b1p", "proj+n1"), ("chunk", "proj+n1"), ("tok_e", "proj+n1"), ("noclamp", "proj+n1"), ("b1p", "proj+skip+tap"),
                      ("chunk", "proj+skip+tap"), ("noclamp", "ln"), ("tok_e", "last"), ("halves", "proj+frag"), ("halves", "proj+skip+frag")):
        with pytest.raises(AssertionError):
            check(o, emulate(o, mode, bug=bug))
    # the polynomial: the DD_S_G* literals are the halved coefficients of gemm.hip gelu_erf4 (tests/test_gemm_path.py), within GELU_POLY over +-16
    coef, hi = gelu_literals()
    gemm = (7.331517960e-08, -4.544908101e-06, 1.213693460e-04, -1.863093246e-03, 1.863326334e-02, -1.314395642e-01, 7.973534865e-01)
    assert hi == np.float32(3.8) and [float(c) for c in coef] == [float(np.float32(0.5) * np.float32(c)) for c in gemm]
    v = np.linspace(-16, 16, 200001).astype(np.float32)
    assert np.abs(gelu_poly(v).astype(np.float64) - gelu_exact(v)).max() <= GELU_POLY
    assert np.abs(gelu_poly(v, clamp=False).astype(np.float64) - gelu_exact(v)).max() > 1.0


# ---------------------------------------------------------------------------------------------------------------- GPU tests
@gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_block_tail_against_float64_reference(case):
    geom, D, mode, dense = case
    o = ops_for(*geom, D, dense)
    check(o, run(o, mode))


@gpu
def test_refused_combinations_launch_nothing():
    """fragment order needs whole 32-row groups of patch rows (300 patches: refused, which is why that geometry has no proj+frag case); the
    caller's arrays are not written"""
    o = ops_for(1, 300, 0, 512)
    res = run(o, "proj+frag")
    assert res["status"] == DD_ERR_UNSUPPORTED
    assert not res["frag"].any() and not res["ln"].any() and not res["out"].any() and not res["slab"].any()
    assert np.array_equal(res["xres"][:o.M], o.x0)


@gpu
@pytest.mark.parametrize("mode", ["proj+frag", "proj+skip+tap"])
def test_an_image_computes_the_same_alone_and_inside_a_batch(mode):
    """which path a row takes depends only on its token index (mlp_fused.hip header): images 0, 3 (straddles tiles 0 / 1) and 16 (the ragged fifth
    tile, the second hidden-split tile) of the B = 17 launch equal the same image launched alone, for every output"""
    o = ops_for(*G17, 512)
    big = run(o, mode)
    N, L, D = o.N, o.L, o.D
    for b in (0, 3, 16):
        one = run(o.image(b), mode)
        rows = slice(b * L, (b + 1) * L)
        for k in ("xres", "out", "ln", "tap"):
            if big[k] is not None:
                assert same_bytes(big[k][rows], one[k][:L]), (mode, b, k)
        if big["frag"] is not None:
            assert same_bytes(big["frag"][b * N * D: (b + 1) * N * D], one["frag"][: N * D]), (mode, b, "frag")


@gpu
def test_modes_that_only_move_a_store_do_not_change_a_bit():
    """fragment order against row-major norm1 (the epilogue's arithmetic is the same, only the store address differs; the skip rows' column-split
    form runs the same MFMA sequence per column tile as the form with the LayerNorm); the tap against no tap; the last block's launch against
    the full one on the patch rows"""
    o = ops_for(*G17, 512)
    patch, M, D = o.patch, o.M, o.D
    n_main = int(patch.sum())
    for rm, fm in (("proj+n1", "proj+frag"), ("proj+skip+n1", "proj+skip+frag")):
        a, b = run(o, rm), run(o, fm)
        assert same_bytes(a["xres"], b["xres"]), (rm, fm)
        assert same_bytes(unfrag(b["frag"], n_main // 32, D), a["ln"][:M][patch]), (rm, fm)
        assert same_bytes(a["out"], b["out"])
    t, n = run(o, "proj+skip+tap"), run(o, "proj+skip+n1")
    assert same_bytes(t["xres"], n["xres"]) and same_bytes(t["ln"], n["ln"]) and same_bytes(t["out"], n["out"])
    tf, nf = run(o, "proj+skip+tap+frag"), run(o, "proj+skip+frag")
    assert same_bytes(tf["xres"], nf["xres"]) and same_bytes(tf["frag"], nf["frag"]) and same_bytes(tf["tap"], t["tap"])
    full, last = run(o, "proj"), run(o, "last")
    assert same_bytes(full["xres"][:M][patch], last["xres"][:M][patch])
    check(o, full)


@gpu
@pytest.mark.parametrize("mode", ["proj+frag", "proj+skip+tap", "proj+skip+qkv", "plain"])
def test_poison_does_not_reach_an_output(mode):
    """a second launch whose slab buffer and padding rows hold another fill pattern (0x7F bytes: finite, huge) returns the same bytes"""
    o = ops_for(*G17, 512)
    a, b = run(o, mode), run(o, mode, poison=0x7F)
    M = o.M
    used = a["plan"][1] * a["plan"][2] * a["plan"][3]
    assert same_bytes(a["xres"][:M], b["xres"][:M]) and same_bytes(a["slab"][:used], b["slab"][:used])
    for k in ("out", "ln", "frag", "tap", "qkv"):
        if a[k] is not None:
            assert same_bytes(a[k], b[k]), (mode, k)
    check(o, b)


@gpu
@pytest.mark.parametrize("M,extras,geom,skip", [(130, 0, (1, 130, 0), False), (10, 1, (5, 1, 1), False), (10, 1, (5, 1, 1), True)],
                         ids=["M130-E0", "M10-E1", "M10-E1-skip"])
def test_dd_dev_mlp_and_dd_dev_block_tail_return_the_same_bytes(M, extras, geom, skip):
    """the two entry points take their launch arguments from one plan (csrc/launch_args.h), so the same rows come back bit for bit: two main tiles,
    the second ragged; the hidden-split tiles and the reduce launch; those again with the next skip_linear.  D = 128, hidden = 256, norm2 in the
    prologue, the projection in front, norm1 behind.  Only the padding differs (dd_dev_mlp: zero rows up to a multiple of 256; dd_dev_block_tail:
    0xFF bytes), so the rows [0, M) are compared; a SKIP launch writes the bf16 copy of the extra-token rows only, and the patch rows of each
    entry's buffer keep what it was filled with"""
    from duodiff_amd.engine import Context
    ctx = Context.get()
    B, N, E = geom
    D, hidden = 128, 256
    assert B * (N + E) == M and E == extras
    r = np.random.default_rng([M, extras, int(skip)])
    f = lambda *shape, s=1.0: (s * r.standard_normal(shape)).astype(np.float32)
    w1, b1, w2, b2 = f(hidden, D, s=0.05), f(hidden, s=0.2), f(D, hidden, s=0.05), f(D, s=0.2)
    x, ao, wp, bp = f(M, D, s=1.5) + np.float32(0.3), f(M, D), f(D, D, s=0.05), f(D, s=0.2)
    ln_in, ln_out = (np.stack([1 + 0.1 * r.standard_normal(D), 0.05 * r.standard_normal(D)]).astype(np.float32) for _ in range(2))
    sk, ws, bs = (f(M, D, s=1.2), f(D, 2 * D, s=0.04), f(D, s=0.2)) if skip else (None, None, None)
    ms = C.c_float(0)
    # dd_dev_mlp: extras > 0: M / (1 + extras) images of one patch token; extras == 0: one image of M patch tokens
    got, out, hout = x.copy(), np.zeros((M, D), np.uint16), np.zeros((M, D), np.uint16)
    ctx.check(ctx.lib.dd_dev_mlp(ctx.handle, M, D, hidden, extras, P(x), P(w1), P(b1), P(w2), P(b2), P(got), P(out), P(ln_in), P(ln_out), P(hout), 0,
                                 None, C.byref(ms), P(ao), P(wp), P(bp), P(sk), P(ws), P(bs), None, None))
    # dd_dev_block_tail: the same rows as B images of N patch tokens behind E extra tokens
    Mo = round_up(M, 256) + 8
    xres = np.full((Mo, D), NAN32, np.uint32).view(np.float32)
    xres[:M] = x
    tout, tln = np.zeros((Mo, D), np.uint16), np.zeros((Mo, D), np.uint16)
    srows = (B * E + 31) // 32 * 16 * 32 + 8
    slab = np.zeros((srows, D), np.float32)
    ctx.check(ctx.lib.dd_dev_block_tail(ctx.handle, B, N, E, D, hidden, 0, 0xFF, None, P(w1), P(b1), P(w2), P(b2), P(ln_in), P(ao), P(wp), P(bp),
                                        P(ln_out), P(sk), P(ws), P(bs), None, P(xres), P(tout), P(tln), None, None, None, P(slab), srows, None, 0,
                                        None, C.byref(ms)))
    patch = (np.arange(M) % (N + E)) >= E
    assert np.isfinite(got).all()
    assert same_bytes(got, xres[:M]), "xres"
    assert same_bytes(hout, tln[:M]), "ln_out"
    written = ~patch if skip else np.ones(M, bool)
    assert same_bytes(out[written], tout[:M][written]), "bf16 copy"
    assert not out[~written].any() and untouched(tout[:M][~written]), "a SKIP launch wrote the bf16 copy of patch rows"
    if E:
        assert not np.array_equal(out[~patch], np.zeros_like(out[~patch])), "the extra-token rows' bf16 copy was not written"
