"""What the per-element kernel tests share (test_attention, test_block_tail, test_frag_handoff, test_gemm_path, test_row_kernels,
test_qkv_attention, test_mlp_fused, test_pag, test_head_dec): bf16 arithmetic on the host, the elementwise gate, the constants of the bounds,
the LayerNorm bound of the GEMM-path tests and the MFMA fragment order.  tests/test_kernel_support.py (CPU) pins every piece of it."""
import numpy as np

from duodiff_amd import _lib
from oracle.uvit_oracle import layer_norm

PREC_BF16, PREC_FP32 = _lib.DD_PREC_BF16, _lib.DD_PREC_FP32
FP32_REL = 2.0 ** -16          # fp32 accumulation of bf16 products (K / 16 MFMA partial sums, + bias, + x)
PARITY_REL = 2.0 ** -20        # fp32 parity mode
GELU_POLY = 2.41e-4            # |gelu_erf4 (bf16 mode) - exact GELU| for |v| <= 16 (gemm.hip);
#                                the same polynomial in mlp_fused.hip: "GELU abs error <= 2.4e-4, same coefficients as the GEMM epilogue"
GELU_SLOPE = 1.13              # max |d gelu / dv|
NAN32, NAN16 = 0xFFFFFFFF, 0xFFFF


# ---------------------------------------------------------------------------------------------------------------- bf16 on the host
def bf16_bits(a):
    """fp32 -> the bits of bf16 (round to nearest even), as host_f2bf"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def from_bf16_bits(b):
    return (np.ascontiguousarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16(a):
    """fp32 -> bf16 (round to nearest even) -> fp32"""
    return from_bf16_bits(bf16_bits(a))


def ulp_bf16(y):
    """one bf16 ulp at bf16(y) (0 at 0: the fp32 term covers it)"""
    yb = np.abs(bf16(np.asarray(y, np.float32))).astype(np.float64)
    _, e = np.frexp(yb)
    return np.where(yb == 0, 0.0, np.ldexp(1.0, e - 8))


def gelu_exact(v):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(v, np.float64))
    return (0.5 * t * (1.0 + torch.special.erf(t / np.sqrt(2.0)))).numpy()


# ---------------------------------------------------------------------------------------------------------------- the gate
def gate(got, want, tol, what):
    """elementwise |got - want| <= tol (tol broadcast to want's shape); NaN fails.  Returns the largest error / bound ratio, 0.0 of nothing."""
    got, want = np.asarray(got, np.float64), np.asarray(want)
    if got.size == 0:
        return 0.0
    tol = np.broadcast_to(np.asarray(tol, np.float64), want.shape)
    err = np.abs(got - want)
    bad = ~(err <= tol)
    ratio = err / np.maximum(tol, 1e-300)
    if bad.any():
        i = tuple(map(int, np.argwhere(bad)[0]))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements out of bound; first at {i}: got {float(got[i])!r}, want {float(want[i])!r}, "
                             f"bound {float(tol[i])!r}; largest error / bound {np.where(np.isnan(ratio), np.inf, ratio).max():.3f}")
    return float(ratio.max())


def ln_ref_and_tol(x, g, b):
    """LayerNorm of fp32 rows x (the kernel's own) and the bf16 bound: one ulp + 2^-16 of the rows' scale in units of their spread"""
    want = layer_norm(x.astype(np.float32), g, b).astype(np.float64)
    x64 = x.astype(np.float64)
    rstd = 1.0 / np.sqrt(x64.var(-1, keepdims=True) + 1e-5)
    scale = np.abs(x64).max(-1, keepdims=True) * rstd
    return want, ulp_bf16(want) + FP32_REL * (scale * np.abs(g) + np.abs(b)) + 1e-30


# ---------------------------------------------------------------------------------------------------------------- buffers and the GPU call
def round_up(v, m):
    return (v + m - 1) // m * m


def untouched(a):
    """every byte still holds the 0xFF the entry point filled the buffer with"""
    return bool(np.all(np.ascontiguousarray(a).view(np.uint8) == 0xFF))


def ctx():
    from duodiff_amd.engine import Context
    return Context.get()


def P(a):
    return None if a is None else a.ctypes.data


# ---------------------------------------------------------------------------------------------------------------- the fragment order
# include/duodiff_dev.h, dd_dev_block_tail_frag: a fragment buffer holds patch rows only, group = patch row / 32 counted over all images;
#   bf16 buffers: element ((group (D / 16) + ks) 64 + lane) 8 + j = column 16 ks + 8 (lane >> 5) + j of patch row 32 group + (lane & 31);
#   fp32 buffers: element (((group (D / 32) + t) 4 + g) 64 + lane) 4 + e = column 32 t + 8 g + 4 (lane >> 5) + e of that row.
# The bf16 order is also MlpFusedArgs::ln_out_frag's, layernorm_kernel's and QkvAttnArgs::out_frag's.
def frag16_index(rows, D):
    """[rows, D]: the flat element index of (patch row p, column c) in a bf16 fragment buffer"""
    p, c = np.arange(rows)[:, None], np.arange(D)[None, :]
    group, ks, lane, j = p // 32, c // 16, p % 32 + 32 * (c % 16 // 8), c % 8
    return ((group * (D // 16) + ks) * 64 + lane) * 8 + j


def frag32_index(rows, D):
    """[rows, D]: the same of an fp32 fragment buffer"""
    p, c = np.arange(rows)[:, None], np.arange(D)[None, :]
    group, t, g, lane, e = p // 32, c // 32, c % 32 // 8, p % 32 + 32 * (c % 8 // 4), c % 4
    return (((group * (D // 32) + t) * 4 + g) * 64 + lane) * 4 + e


def to_frag(rows_, D, swap_halves=False, index=frag16_index):
    """rows [groups 32, D] -> fragment order, flat; swap_halves: the bug of a bf16 store that exchanges the two lane halves"""
    idx = index(rows_.shape[0], D)
    if swap_halves:
        assert index is frag16_index
        idx = idx ^ (32 * 8)                # lane ^ 32
    out = np.empty(rows_.size, rows_.dtype)
    out[idx] = rows_
    return out


def unfrag(fr, groups, D, index=frag16_index):
    """the first `groups` 32-row groups of a fragment buffer -> [groups 32, D] rows"""
    return fr.reshape(-1)[: groups * 32 * D][index(groups * 32, D)]


# ---------------------------------------------------------------------------------------------------------------- the output head + step launch
# What tests/test_final_step.py (GPU, through dd_dev_final) compares step.hip's final_tiled_kernel with: the head in float64 with its derived
# bound, step_update.h restated in float32, and the kernel's Philox draw from integer numpy.  Each carries one-line switches for the
# deliberate errors the CPU mutant tests of tests/test_kernel_support.py prove the test inputs can see.
F32 = np.float32
U24 = 2.0 ** -24               # the unit roundoff of fp32


def final_unpatchify64(dec, B, L, extras, C, chan_first=False):
    """the patch rows of dec [B L, P P C] -> float64 [B, C, S, S]; chan_first: the bug of reading a patch as (C p1 p2)"""
    from oracle.uvit_oracle import unpatchify
    rows = np.asarray(dec, np.float64).reshape(B, L, -1)[:, extras:]
    if chan_first:
        P = int(round((rows.shape[-1] // C) ** 0.5))
        rows = rows.reshape(B, L - extras, C, P, P).transpose(0, 1, 3, 4, 2).reshape(B, L - extras, -1)
    return unpatchify(rows, C)


def final_conv64(u, w, b, taps_transposed=False, edge_shift=False):
    """3x3 conv, pad 1, of u [B, C, S, S] with w [C, C, 3, 3] + b in float64 -> (eps, mag), mag = |b| + sum |w| |u| (what the rounding
    bound scales with).  taps_transposed: ky and kx swapped; edge_shift: a pixel in the last column of a 16-wide tile reads its right-hand
    taps one pixel further right (a halo column filled from the wrong pixel)"""
    u, w, b = np.asarray(u, np.float64), np.asarray(w, np.float64), np.asarray(b, np.float64)
    if taps_transposed:
        w = w.transpose(0, 1, 3, 2)
    B, C, S, _ = u.shape
    up = np.zeros((B, C, S + 2, S + 3))
    up[:, :, 1:S + 1, 1:S + 1] = u
    eps = np.zeros((B, C, S, S)) + b[None, :, None, None]
    mag = np.zeros((B, C, S, S)) + np.abs(b)[None, :, None, None]
    for ky in range(3):
        for kx in range(3):
            win = up[:, :, ky:ky + S, kx:kx + S]
            if edge_shift and kx == 2:
                win = win.copy()
                win[..., 15::16] = up[:, :, ky:ky + S, 3:3 + S][..., 15::16]
            eps += np.einsum("bchw,oc->bohw", win, w[:, :, ky, kx])
            mag += np.einsum("bchw,oc->bohw", np.abs(win), np.abs(w[:, :, ky, kx]))
    return eps, mag


def final_eps64(dec, wconv, bconv, B, C, S, P, L, extras, *, dec2=None, wconv2=None, bconv2=None, L2=0, extras2=0, pair_B=0, scale=0.0,
                layer_B=0, w_stride=0, b_stride=0, mutant=None):
    """eps of the launch in float64 and its per-element bound.  Plain: the conv of the unpatchified rows (layer_B > 0: layer b // layer_B's
    own weights).  Guided: c + s (c - u), u from the twin rows of dec under the same conv (pair_B) or from dec2 under wconv2 / bconv2.
    The bound, derived: an fmaf chain of 9 C terms on the bias rounds once per term, so |error| <= (9 C + 2) 2^-24 (|b| + sum |w| |u|) per
    pixel (gamma_n <= (n + 2) u for these n); the operands are fp32 and exact in float64.  Guided, the kernel computes d = c - u, p = s d,
    eps = c + p, one rounding each: the errors Ec, Eu of the two convs arrive as (1 + |s|) Ec + |s| Eu, and the three roundings add at most
    2^-24 (2 |s| |d'| + |eps'|) with |d'| <= |c - u| + Ec + Eu and |eps'| <= |eps| + (1 + |s|) Ec + |s| Eu (+ second-order terms: x 1.001).
    mutant: None, "taps", "chan_first", "edge_shift", "same_weights" (the second source convolved with the first source's weights)."""
    pd = P * P * C
    dec = np.asarray(dec).reshape(-1, pd)
    kw = dict(taps_transposed=mutant == "taps", edge_shift=mutant == "edge_shift")
    cf = mutant == "chan_first"
    wconv, bconv = np.asarray(wconv).reshape(-1), np.asarray(bconv).reshape(-1)

    def conv(rows, n, l, e, w, b):
        return final_conv64(final_unpatchify64(rows, n, l, e, C, cf), w.reshape(C, C, 3, 3), b, **kw)

    if layer_B > 0:
        parts = [conv(dec[i * layer_B * L:(i + 1) * layer_B * L], layer_B, L, extras, wconv[i * w_stride:i * w_stride + 9 * C * C],
                      bconv[i * b_stride:i * b_stride + C]) for i in range(B // layer_B)]
        c, mc = (np.concatenate(v) for v in zip(*parts))
    else:
        c, mc = conv(dec[:B * L], B, L, extras, wconv[:9 * C * C], bconv[:C])
    ec = (9 * C + 2) * U24 * mc
    if pair_B > 0:
        u, mu = conv(dec[pair_B * L:2 * pair_B * L], B, L, extras, wconv[:9 * C * C], bconv[:C])
    elif dec2 is not None:
        same = mutant == "same_weights"
        u, mu = conv(np.asarray(dec2).reshape(-1, pd), B, L2, extras2, wconv[:9 * C * C] if same else np.asarray(wconv2).reshape(-1),
                     bconv[:C] if same else np.asarray(bconv2).reshape(-1))
    else:
        return c, ec
    s = abs(float(F32(scale)))
    eu = (9 * C + 2) * U24 * mu
    eps = c + float(F32(scale)) * (c - u)
    lin = (1 + s) * ec + s * eu
    return eps, 1.001 * (lin + U24 * (2 * s * (np.abs(c - u) + ec + eu) + np.abs(eps) + lin))


# ---- step_update.h in numpy: every product and sum rounded to `dtype` on its own, in the header's order (it compiles with fp contract off)
def step_ddpm(x, eps, z, c1, c2, sigma, dtype=F32):
    """x' = c1 (x - c2 eps) [+ sigma z]: mul, sub, mul [, mul, add]; z None: a step without noise"""
    x, eps, c1, c2 = np.asarray(x, dtype), np.asarray(eps, dtype), dtype(c1), dtype(c2)
    with np.errstate(invalid="ignore", over="ignore"):
        v = c1 * (x - c2 * eps)
        if z is not None:
            v = v + dtype(sigma) * np.asarray(z, dtype)
    return v


def step_table(x, m, z, h, a, b, c, d, use_hist, dtype=F32):
    """x' = a x + b m [+ d h if use_hist] [+ c z]; h is not touched without use_hist (0 * NaN is NaN)"""
    x, m = np.asarray(x, dtype), np.asarray(m, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        v = dtype(a) * x + dtype(b) * m
        if use_hist:
            v = v + dtype(d) * np.asarray(h, dtype)
        if z is not None:
            v = v + dtype(c) * np.asarray(z, dtype)
    return v


def step_history(x, m, p, q, dtype=F32):
    """h' = p x + q m (StepRule::history)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return dtype(p) * np.asarray(x, dtype) + dtype(q) * np.asarray(m, dtype)


def step_known(xp, x0, m, ka, kb, z2, dtype=F32):
    """known(): x' where m == 0 bit for bit, else m (ka x0 [+ kb z2 if kb != 0 and z2 is there]) + (1 - m) x'"""
    xp, x0, m = np.asarray(xp, dtype), np.asarray(x0, dtype), np.asarray(m, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        kn = dtype(ka) * x0
        if z2 is not None and dtype(kb) != 0:
            kn = kn + dtype(kb) * np.asarray(z2, dtype)
        mixed = m * kn + (dtype(1) - m) * xp
    return np.where(m == 0, xp, mixed).astype(dtype)


# ---- the device noise: Philox4x32-10 and the Box-Muller of step_update.h philox_normal4
PHILOX_STEP, PHILOX_KNOWN = 0x5EED, 0x6B6E6F77


def philox4x32_10(counter, key):
    """Philox4x32 with 10 rounds (Salmon et al., Random123): counter [..., 4], key [..., 2] of uint32 -> [..., 4] uint32"""
    m32, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    c = [np.asarray(counter, np.uint64)[..., i] & m32 for i in range(4)]
    k = [np.asarray(key, np.uint64)[..., i] & m32 for i in range(2)]
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(0xD2511F53), c[2] * np.uint64(0xCD9E8D57)
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & m32, (p0 >> s32) ^ c[3] ^ k[1], p0 & m32]
        k = [(k[0] + np.uint64(0x9E3779B9)) & m32, (k[1] + np.uint64(0xBB67AE85)) & m32]
    return np.stack(np.broadcast_arrays(*c), -1).astype(np.uint32)


def philox_normal4_ref(seed, pixel, ctr, stream=PHILOX_STEP):
    """the four normals of every pixel id in `pixel` (any shape, up to 64 bits) -> (z [..., 4] float64, ulog [..., 2] float32: the two
    uniforms that go through the logarithm).  Counter (pixel lo, pixel hi, ctr, stream), key (seed lo, seed hi).  The uniforms and the
    two angles are built in float32 exactly as the kernel builds them -- (float)c + 1 and the 2^-32 scale, uint -> float rounding to
    nearest even on both sides, 2 pi (float) times the uniform rounded once -- and sqrt, log, sin, cos are float64 functions of those
    float32 values: what is left against the kernel is the error of its hardware log, sin and cos (and three fp32 roundings)."""
    pixel = np.asarray(pixel, np.uint64)
    seed, m32 = np.uint64(seed), np.uint64(0xFFFFFFFF)
    ctrw = np.uint64(int(ctr) & 0xFFFFFFFF)
    counter = np.stack([pixel & m32, pixel >> np.uint64(32), np.broadcast_to(ctrw, pixel.shape), np.broadcast_to(np.uint64(stream), pixel.shape)], -1)
    c = philox4x32_10(counter, np.array([seed & m32, seed >> np.uint64(32)], np.uint64))
    scale = F32(2.3283064365386963e-10)
    f = c.astype(F32)                                   # uint32 -> float32, round to nearest even
    ua, uc = (f[..., 0] + F32(1)) * scale, (f[..., 2] + F32(1)) * scale
    aa, ac = F32(6.283185307179586) * (f[..., 1] * scale), F32(6.283185307179586) * (f[..., 3] * scale)
    assert ua.dtype == F32 and aa.dtype == F32
    ra, rc = np.sqrt(-2.0 * np.log(ua.astype(np.float64))), np.sqrt(-2.0 * np.log(uc.astype(np.float64)))
    aa, ac = aa.astype(np.float64), ac.astype(np.float64)
    return np.stack([ra * np.cos(aa), ra * np.sin(aa), rc * np.cos(ac), rc * np.sin(ac)], -1), np.stack([ua, uc], -1)


def final_pixel_ids(B, S, b0, transposed=False):
    """[B, S, S] uint64: the id of pixel (y, x) of image b within the whole batch, ((b + b0) S + y) S + x; transposed: the bug x S + y"""
    b, y, x = np.meshgrid(np.arange(B, dtype=np.uint64), np.arange(S, dtype=np.uint64), np.arange(S, dtype=np.uint64), indexing="ij")
    if transposed:
        y, x = x, y
    return ((b + np.uint64(b0)) * np.uint64(S) + y) * np.uint64(S) + x


def final_philox_ref(seed, B, C, S, b0, ctr, stream=PHILOX_STEP, transposed=False):
    """the launch's z (or z2) -> (z [B, C, S, S] float64, near_one [B, C, S, S] bool: the draws whose logarithm's uniform rounds to within
    2^-10 of 1, selected by the reference's uniforms alone)"""
    z, ulog = philox_normal4_ref(seed, final_pixel_ids(B, S, b0, transposed), ctr, stream)
    near = np.repeat(ulog >= F32(1.0 - 2.0 ** -10), 2, -1)          # components 0, 1 share ua; 2, 3 share uc
    return z[..., :C].transpose(0, 3, 1, 2), near[..., :C].transpose(0, 3, 1, 2)


def final_inputs(C, P, S, B, extras, seed, guided=None, extras2=None, layers=1):
    """the operands of a head test: standard-normal decoder rows and conv weights (neither symmetric nor separable), NaN in the rows of the
    extra tokens, which must never be read.  guided "cfg": dec holds 2 B images; "auto": a second source with its own token count and conv.
    layers > 1: B = layers * layer_B images, one conv per layer at strides 9 C C + 5 / C + 3 (the gaps hold NaN)."""
    r = np.random.default_rng(seed)
    g, pd = S // P, P * P * C
    L = extras + g * g

    def rows(n, l, e):
        d = r.standard_normal((n, l, pd)).astype(F32)
        d[:, :e] = np.nan
        return d.reshape(n * l, pd)

    ws, bs = 9 * C * C + 5, C + 3
    w = np.full((layers - 1) * ws + 9 * C * C, np.nan, F32)
    b = np.full((layers - 1) * bs + C, np.nan, F32)
    for i in range(layers):
        w[i * ws:i * ws + 9 * C * C] = r.standard_normal(9 * C * C)
        b[i * bs:i * bs + C] = r.standard_normal(C)
    out = dict(B=B, C=C, S=S, P=P, L=L, extras=extras, dec=rows(2 * B if guided == "cfg" else B, L, extras), wconv=w, bconv=b)
    if layers > 1:
        out.update(layer_B=B // layers, w_stride=ws, b_stride=bs)
    if guided == "cfg":
        out.update(pair_B=B, scale=1.75)
    if guided == "auto":
        e2 = extras2 if extras2 is not None else 3 - extras
        out.update(dec2=rows(B, e2 + g * g, e2), wconv2=r.standard_normal(9 * C * C).astype(F32), bconv2=r.standard_normal(C).astype(F32),
                   L2=e2 + g * g, extras2=e2, scale=-0.625)
    return out


# the shapes of tests/test_final_step.py, here so that the CPU mutant tests judge the very inputs the GPU tests use
FINAL_FORMS = [(3, 4), (3, 2), (4, 2), (1, 1), (2, 2), (3, 1), (4, 4), (1, 8)]      # the three compiled (C, P) forms, then the run-time form
FINAL_SIZES = [8, 16, 24, 32, 48]                                                    # + 64 once, at B = 1, (3, 4)
FINAL_B = 3


def final_head_inputs(C, P, S, guided=None, B=FINAL_B, extras=None):
    """the head test's operands at (C, P, S): extras alternates 1 / 2 with the size, autoguidance takes the other count for its guide"""
    extras = extras if extras is not None else 1 + (S // 8) % 2
    return final_inputs(C, P, S, B, extras, 1000 * C + 100 * P + S + (7 if guided else 0), guided)


# Philox cases: ids across tiles and images, every channel count, a launch that starts at image 5, a seed above 2^32, two counters, the known
# region's stream word, and a pixel id above 2^32 (b0 = 2^20 + 5 at S = 64)
PHILOX_CASES = [
    dict(S=32, B=3, C=3, b0=0, seed=0x1234, ctr=0, z2=False),
    dict(S=24, B=3, C=4, b0=0, seed=(7 << 32) | 0x9ABCDEF1, ctr=0, z2=False),
    dict(S=24, B=3, C=1, b0=5, seed=0x1234, ctr=941, z2=False),
    dict(S=32, B=3, C=3, b0=5, seed=(1 << 32) + 3, ctr=17, z2=False),
    dict(S=24, B=3, C=3, b0=0, seed=0x1234, ctr=17, z2=True),
    dict(S=32, B=3, C=4, b0=5, seed=(7 << 32) | 0x9ABCDEF1, ctr=941, z2=True),
    dict(S=64, B=1, C=3, b0=(1 << 20) + 5, seed=(1 << 63) | 0x55, ctr=3, z2=False),
]
