"""What the per-element kernel tests share (test_attention, test_block_tail, test_frag_handoff, test_gemm_path, test_row_kernels,
test_qkv_attention, test_mlp_fused, test_pag, test_head_dec, test_vae_gemm): bf16 arithmetic on the host, the elementwise gate, the constants of the bounds,
the LayerNorm bound of the GEMM-path tests, the MFMA fragment order, the references of the output head + step launch (test_final_step) and
of the KL-VAE kernels (test_vae_kernels) and of the early-exit probes (test_ee_probes).  tests/test_kernel_support.py (CPU) pins every piece of it."""
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


# ---------------------------------------------------------------------------------------------------------------- the KL-VAE kernels
# What tests/test_vae_kernels.py (GPU, through dd_dev_vae_gather, dd_dev_groupnorm, dd_dev_softmax_rows, dd_dev_vae_input / _output /
# _moments and dd_dev_cast) compares csrc/vae_kernels.hip with: float64 restatements (index arithmetic for the gathers), the inputs of
# every case, and the derived bounds.  The switches (`mutant=`) are the deliberate errors that the CPU tests of tests/test_kernel_support.py
# prove those inputs can see.
VAE_TAIL = 64                  # DD_DEV_VAE_TAIL: canary elements behind every output
VAE_SCALE = 0.18215
GATHER_C = (8, 128)
# (kind, B, H, W): kind 2 = 3x3 im2col, kind 3 = the same through the nearest-2x upsample (H, W: the convolution's size)
GATHER_SHAPES = [(2, 1, 1, 1), (2, 3, 2, 2), (3, 3, 2, 2), (2, 2, 4, 6), (3, 2, 4, 6), (3, 2, 6, 4)]


def vae_kpad(C, prec):
    """9 C rounded up to the GEMM k-tile (128 bytes of elements), as dd_vae_finalize pads a conv's K"""
    return round_up(9 * C, 64 if prec == "bf16" else 32)


def gather_input(kind, B, H, W, C):
    """the source of a gather case, exact in bf16: [B, H, W, C], or [B, H / 2, W / 2, C] for the upsample"""
    r = np.random.default_rng(10000 * kind + 1000 * B + 100 * H + 10 * W + C)
    s = 2 if kind == 3 else 1
    return r.integers(-64, 64, (B, H // s, W // s, C)).astype(F32) / 8.0


def im2col3x3_ref(src, up, kpad, mutant=None):
    """rows [B H W, kpad] of the 3x3 / pad 1 im2col over NHWC src, columns (ky, kx, c), [9 C, kpad) zero; up: through np.repeat by 2.
    mutant: "taps" (ky, kx transposed), "half_x" (the upsample's / 2 dropped along x: column x reads source column min(x, Ws - 1)),
    "edge" (a pad tap reads the clamped edge pixel instead of zero)"""
    src = np.asarray(src)
    img = src
    if up:
        img = np.repeat(src, 2, axis=1)
        img = np.repeat(img, 2, axis=2) if mutant != "half_x" else img[:, :, np.minimum(np.arange(2 * src.shape[2]), src.shape[2] - 1)]
    B, H, W, C = img.shape
    padded = np.pad(img, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="edge" if mutant == "edge" else "constant")
    out = np.zeros((B, H, W, kpad), src.dtype)
    for ky in range(3):
        for kx in range(3):
            t = kx * 3 + ky if mutant == "taps" else ky * 3 + kx
            out[..., t * C:(t + 1) * C] = padded[:, ky:ky + H, kx:kx + W]
    return out.reshape(B * H * W, kpad)


# ---- GroupNorm(32, eps 1e-6) [+ swish] over NHWC rows x [B HW, C]
GN_SHAPES = [(2, 64, 128), (2, 9, 256), (3, 300, 512), (2, 576, 128), (1, 64, 384)]      # (B, HW, C)
GN_PAIRS = [(0.0, 1.0), (10.0, 1.0), (100.0, 1.0), (30.0, 0.1)]                           # (mean, std) of an (image, group)
GN_MARGIN = 8.0                # an fp32 kernel against torch's fp32 group_norm: summation order and expf (as test_encode_moments_fp32)


def gn_pair_index(B, C):
    """[B, C]: which of GN_PAIRS a channel's group has in an image; rotated by the image, so a cross-image mix-up shows"""
    g = np.arange(C) // (C // 32)
    return (g[None, :] + np.arange(B)[:, None]) % len(GN_PAIRS)


def gn_inputs(B, HW, C, const=False):
    """x [B HW, C] fp32, gamma, beta.  const: (image 0, group 7) holds 123.456 and (image B - 1, group 5) holds 0.1 everywhere"""
    r = np.random.default_rng(100000 * B + 100 * HW + C + (1 if const else 0))
    k = gn_pair_index(B, C)
    mean, std = np.array(GN_PAIRS)[k, 0], np.array(GN_PAIRS)[k, 1]
    x = (mean[:, None, :] + std[:, None, :] * r.standard_normal((B, HW, C))).astype(F32)
    if const:
        cpg = C // 32
        x[0, :, 7 * cpg:8 * cpg] = F32(123.456)
        x[B - 1, :, 5 * cpg:6 * cpg] = F32(0.1)
    gamma = (1.0 + 0.5 * r.standard_normal(C)).astype(F32)
    beta = r.standard_normal(C).astype(F32)
    return x.reshape(B * HW, C), gamma, beta


def _swish(y):
    with np.errstate(over="ignore"):
        return y / (1.0 + np.exp(-y))


def groupnorm_ref(x, gamma, beta, B, HW, C, swish, mutant=None):
    """float64 GroupNorm(32 groups over C / 32 consecutive channels, biased variance, eps 1e-6) * gamma + beta [-> y sigmoid(y)].
    mutant: "group_map" (a channel's group taken as its float4 column, (c // 4) % 32: right at C = 128 only), "drop_tail" (the partial last
    256-pixel chunk left out of the element count)"""
    x64 = np.asarray(x, np.float64).reshape(B, HW, C)
    gid = (np.arange(C) // 4) % 32 if mutant == "group_map" else np.arange(C) // (C // 32)
    hw_n = HW // 256 * 256 if mutant == "drop_tail" and HW > 256 else HW
    y = np.empty_like(x64)
    for g in range(32):
        m = gid == g
        xg = x64[:, :, m]
        n = float(hw_n * m.sum())
        mean = xg.sum((1, 2), keepdims=True) / n
        var = np.maximum((xg * xg).sum((1, 2), keepdims=True) / n - mean * mean, 0.0) if mutant == "drop_tail" else xg.var((1, 2), keepdims=True)
        y[:, :, m] = (xg - mean) / np.sqrt(var + 1e-6)
    y = y * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)
    return (_swish(y) if swish else y).reshape(B * HW, C)


def groupnorm_torch(x, gamma, beta, B, HW, C, swish, dtype):
    """torch's F.group_norm (+ F.silu) on the CPU in `dtype` -> float64 rows [B HW, C]"""
    import torch
    import torch.nn.functional as TF
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(x).reshape(B, HW, C).transpose(0, 2, 1))).to(dtype).reshape(B, C, HW, 1).contiguous()
    y = TF.group_norm(t, 32, torch.from_numpy(gamma).to(dtype), torch.from_numpy(beta).to(dtype), eps=1e-6)
    y = TF.silu(y) if swish else y
    return y.reshape(B, C, HW).permute(0, 2, 1).reshape(B * HW, C).to(torch.float64).numpy()


def groupnorm_emulated(x, gamma, beta, B, HW, C, swish, pivot):
    """the three kernels in numpy float32, in their summation order: per 256-pixel chunk every thread adds its pixels in turn, the four lanes
    of a float4 pair up, one thread per group adds the chunk's columns in turn; the chunks are combined in double; apply in float32.
    pivot False: the sums of x and x^2 (the one-pass formula q / n - mean^2).  pivot True: the sums of d and d^2, d = x - the group's first
    channel at the image's first pixel, mean = pivot + s / n, var = q / n - (s / n)^2."""
    x3 = np.asarray(x, F32).reshape(B, HW, C)
    c4, cpg = C // 4, C // 32
    rows, w = 256 // c4, c4 // 32
    chunks = (HW + 255) // 256
    S, Q = np.zeros((B, 32)), np.zeros((B, 32))
    pv = x3[:, 0, ::cpg].copy() if pivot else np.zeros((B, 32), F32)                     # [B, 32]
    for ch in range(chunks):
        xc = x3[:, ch * 256:min(HW, ch * 256 + 256)] - np.repeat(pv, cpg, axis=1)[:, None, :]
        xc = xc.astype(F32).reshape(B, -1, c4, 4)
        s, q = np.zeros((B, rows, c4, 4), F32), np.zeros((B, rows, c4, 4), F32)
        for k in range(0, xc.shape[1], rows):
            v = xc[:, k:k + rows]
            s[:, :v.shape[1]] += v
            q[:, :v.shape[1]] += v * v
        ss, sq = (s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3]), (q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])      # [B, rows, c4]
        a, b2 = np.zeros((B, 32), F32), np.zeros((B, 32), F32)
        for r in range(rows):
            for k in range(w):
                a += ss[:, r, k::w]
                b2 += sq[:, r, k::w]
        S += a
        Q += b2
    n = float(HW * cpg)
    ds = S / n
    mean = (pv.astype(np.float64) + ds).astype(F32)
    rstd = (1.0 / np.sqrt(np.maximum(Q / n - ds * ds, 0.0) + 1e-6)).astype(F32)
    t = (x3 - np.repeat(mean, cpg, axis=1)[:, None, :]) * np.repeat(rstd, cpg, axis=1)[:, None, :] * np.asarray(gamma, F32) + np.asarray(beta, F32)
    t = t.astype(F32)
    if swish:
        t = (t / (F32(1.0) + np.exp(-t, dtype=F32))).astype(F32)
    return t.reshape(B * HW, C)


_gn_cache = {}


def gn_case(B, HW, C, swish, const=False):
    """dict of a GroupNorm case, computed once: the inputs, want (torch float64), e32 [B HW, C] = per element the largest error of torch's
    fp32 group_norm (+ silu) against float64 among the elements of the case whose (image, group) has the same (mean, std) pair, and
    e32_case, the largest over the case.  A quantity of the reference alone."""
    key = (B, HW, C, bool(swish), const)
    if key not in _gn_cache:
        import torch
        x, gamma, beta = gn_inputs(B, HW, C, const)
        want = groupnorm_torch(x, gamma, beta, B, HW, C, swish, torch.float64)
        e = np.abs(groupnorm_torch(x, gamma, beta, B, HW, C, swish, torch.float32) - want)
        cls = np.broadcast_to(gn_pair_index(B, C)[:, None, :], (B, HW, C)).reshape(B * HW, C)
        e32 = np.zeros_like(want)
        for k in range(len(GN_PAIRS)):
            e32[cls == k] = e[cls == k].max()
        _gn_cache[key] = dict(x=x, gamma=gamma, beta=beta, want=want, e32=e32, e32_case=float(e.max()), cls=cls)
    return _gn_cache[key]


def gn_tol(case, prec):
    """fp32: 8 e32; bf16: one ulp of the result + 8 e32.  e32 is taken per (mean, std) pair, never above the case's own e32"""
    t = GN_MARGIN * case["e32"]
    return t + ulp_bf16(case["want"]) if prec == "bf16" else t


# ---- softmax over rows
SOFTMAX_SHAPES = [(1, 64), (5, 64), (6, 576), (3, 1024), (7, 100), (2, 1)]      # (rows, n)
SOFTMAX_SCALE = F32(1.0 / np.sqrt(512.0))


def softmax_inputs(rows, n):
    """scores [rows, n] fp32; row i is of kind i % 4: Gaussian of std 40; one dominant entry in the last column, the rest underflowing;
    constant; a permutation of a ramp whose scaled values reach +-80"""
    r = np.random.default_rng(1000 * rows + n)
    s = (40.0 * r.standard_normal((rows, n))).astype(F32)
    for i in range(rows):
        if i % 4 == 1:
            s[i, -1] = 4000.0
        elif i % 4 == 2:
            s[i] = 7.3
        elif i % 4 == 3:
            s[i] = r.permutation(np.linspace(-80.0, 80.0, n) / float(SOFTMAX_SCALE)).astype(F32)
    return s


def softmax_ref(s, scale, prec="fp32", mutant=None):
    """(p, tol): softmax(a) in float64, a = s * scale formed in float64 from the fp32 operands, and the elementwise bound.
    Derivation (u = 2^-24).  The kernel forms t_j = fl(s_j scale), d_j = fl(t_j - mx) and e_j = expf(d_j); softmax does not change under a
    common shift, so mx's own error cancels and the argument is off by at most u |a_j| + u |d_j| <= 2 u (|a_j| + |a_max|); expf is allowed
    4 ulp: e_j has relative error E_j u, E_j = 2 (|a_j| + |a_max|) + 4.  The sum adds ceil(n / 64) terms per lane and 6 shuffle levels, one
    rounding each, and inherits the terms' errors weighted by p: relative error (sum_k p_k E_k + ceil(n / 64) + 6) u.  1 / sum and the
    product round once each.  Second-order terms: x 1.01.  A flushed denormal (an expf below 2^-126, times 1 / sum <= 1): + 2^-126.
    bf16 output: + one bf16 ulp.  mutant: "no_scale" (a = s), "drop_tail" (the elements behind the last whole 64 left out of the sum)"""
    a = np.asarray(s, np.float64) * (1.0 if mutant == "no_scale" else float(F32(scale)))
    amax = a.max(-1, keepdims=True)
    e = np.exp(a - amax)
    n = a.shape[-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        p = e / (e[:, :n // 64 * 64] if mutant == "drop_tail" else e).sum(-1, keepdims=True)
    E = 2.0 * (np.abs(a) + np.abs(amax)) + 4.0
    tol = 1.01 * p * U24 * (E + (p * E).sum(-1, keepdims=True) + -(-n // 64) + 6 + 2) + 2.0 ** -126
    return p, tol + ulp_bf16(p) if prec == "bf16" else tol


# ---- the point-wise kernels
def fma_chain64(v, w, b, n_extra=0):
    """(y, tol): y[..., o] = b[o] + sum_c w[o, c] v[..., c] in float64 and the bound of an fmaf chain of n = w.shape[1] terms started on
    the bias: term c passes through n - c roundings and the bias through n, so |error| <= n u (|b| + sum |w| |v|) to first order;
    (n + 3) u covers the higher orders (gamma_n <= (n + 3) u here) with room; n_extra: roundings the operands v already carry"""
    v, w, b = np.asarray(v, np.float64), np.asarray(w, np.float64), np.asarray(b, np.float64)
    y = v @ w.T + b
    mag = np.abs(v) @ np.abs(w).T + np.abs(b)
    return y, (w.shape[1] + 3 + n_extra) * U24 * mag


VAE_INPUT_SHAPES = [(3, 5), (2, 300)]      # (B, HW)


def vae_input_case(B, HW):
    r = np.random.default_rng(10 * HW + B)
    return dict(B=B, HW=HW, z=r.standard_normal((B, 4, HW)).astype(F32), w=r.standard_normal((4, 4)).astype(F32),
                b=r.standard_normal(4).astype(F32), inv_scale=F32(1.0 / VAE_SCALE))


def vae_input_ref(z, w, b, inv_scale, mutant=None):
    """(out [B HW, 4], tol): post_quant_conv(inv_scale z) in float64, inv_scale at its fp32 value; z inv_scale rounds once before the chain.
    mutant: "w_transposed" """
    v = np.asarray(z, np.float64).transpose(0, 2, 1).reshape(-1, 4) * float(F32(inv_scale))
    return fma_chain64(v, np.asarray(w).T if mutant == "w_transposed" else w, b, n_extra=1)


def vae_output_ref(inp, B, C, HW, ldc):
    """NHWC rows [B HW, ldc] -> NCHW [B, C, HW] of the first C channels"""
    return np.ascontiguousarray(np.asarray(inp).reshape(B, HW, ldc)[:, :, :C].transpose(0, 2, 1))


VAE_MOMENTS_SHAPES = [(3, 5), (2, 300)]      # (B, HW)


def vae_moments_case(B, HW):
    """h [B HW, 8], w, b, eps: h solves w h + b = target, so the log-variances (channels 4..7) cover [-45, 35]: below -30, above 20, between"""
    r = np.random.default_rng(100 * HW + B)
    w = (r.standard_normal((8, 8)) + 2.0 * np.eye(8)).astype(F32)
    b = r.standard_normal(8).astype(F32)
    target = np.concatenate([2.0 * r.standard_normal((B * HW, 4)), r.uniform(-45.0, 35.0, (B * HW, 4))], axis=1)
    target[0, 4:] = (-44.0, -29.0, 19.0, 34.0)
    h = np.ascontiguousarray(np.linalg.solve(w.astype(np.float64), (target - b).T).T, F32)
    return dict(B=B, HW=HW, h=h, w=w, b=b, eps=r.standard_normal((B, 4, HW)).astype(F32))


def vae_moments_ref(h, w, b, eps, B, HW, mutant=None):
    """(moments [B, 8, HW], tol_m, z [B, 4, HW], tol_z) in float64: quant_conv as an fmaf chain of 8 terms, then
    z = SCALE (mean + exp(0.5 clamp(logvar, -30, 20)) eps), or SCALE mean without eps (the mode).
    The bound of z: the sample's own arithmetic on the kernel's fp32 moments is within 4 u SCALE (|mean| + std |eps|) (the rounding of
    std eps, of the sum, of the product with SCALE, the correctly rounded exp and the fp32 value of SCALE: _sample_bound of
    tests/test_vae_encode.py); the moments' errors dm arrive through dz = SCALE (dmean + 1/2 std |eps| dlogvar) (the clamp has slope <= 1;
    exp(x / 2) has derivative std / 2; x 1.001 for the second order).
    mutant: "w_transposed", "no_clamp", "logvar_from_mean" (z takes its log-variance from the mean channels)"""
    m, tol_m = fma_chain64(h, np.asarray(w).T if mutant == "w_transposed" else w, b)
    m = m.reshape(B, HW, 8).transpose(0, 2, 1)
    tol_m = tol_m.reshape(B, HW, 8).transpose(0, 2, 1)
    mean, lv = m[:, :4], (m[:, :4] if mutant == "logvar_from_mean" else m[:, 4:])
    scale = float(F32(VAE_SCALE))
    if eps is None:
        return m, tol_m, scale * mean, 4 * U24 * scale * np.abs(mean) + 1.001 * scale * tol_m[:, :4]
    ae = np.abs(np.asarray(eps, np.float64))
    std = np.exp(0.5 * (lv if mutant == "no_clamp" else np.clip(lv, -30.0, 20.0)))
    z = scale * (mean + std * np.asarray(eps, np.float64))
    tol_z = 4 * U24 * scale * (np.abs(mean) + std * ae) + 1.001 * scale * (tol_m[:, :4] + 0.5 * std * ae * tol_m[:, 4:])
    return m, tol_m, z, tol_z


def cast_inputs():
    """fp32 values for the cast: normals over 2^+-20; exact round-to-even ties (low half 0x8000) above even and odd upper halves of both
    signs, and their neighbours one fp32 ulp either side; +-0.  The count is no multiple of 256."""
    r = np.random.default_rng(3)
    normals = (r.standard_normal(1000) * 2.0 ** r.integers(-20, 21, 1000)).astype(F32)
    hi = np.concatenate([np.arange(0x3500, 0x3600), np.arange(0x4900, 0x4A00)]).astype(np.uint32)      # exponents 2^-21.. and 2^19..
    ties = (np.concatenate([hi, hi | 0x8000]) << 16) | 0x8000
    x = np.concatenate([normals, np.concatenate([ties, ties - 1, ties + 1, np.array([0, 0x80000000], np.uint32)]).view(F32)])
    assert x.size % 256 != 0
    return x


# ---- the GPU calls (tests marked gpu only)
def _prec(prec):
    return (PREC_BF16, np.uint16) if prec == "bf16" else (PREC_FP32, F32)


def vae_gather(kind, prec, B, H, W, C, src):
    """dd_dev_vae_gather -> (rows [B H W + 64, kpad] of bf16 bits / fp32, kpad); src fp32, exact in bf16"""
    c = ctx()
    code, dt = _prec(prec)
    kpad = vae_kpad(4 if kind == 1 else C, prec)
    rows = B * H * W
    dst = np.zeros((rows + VAE_TAIL) * kpad, dt)
    src = np.ascontiguousarray(src, F32)
    src = bf16_bits(src) if prec == "bf16" and kind != 1 else src
    c.check(c.lib.dd_dev_vae_gather(c.handle, kind, code, B, H, W, C, P(src), P(dst), dst.nbytes, None))
    return dst.reshape(rows + VAE_TAIL, kpad), kpad


def run_groupnorm(prec, B, HW, C, swish, x, gamma, beta):
    """dd_dev_groupnorm -> (out [B HW C + TAIL] as float64 values of the bf16 bits / fp32, the raw output, the scratch)"""
    c = ctx()
    code, dt = _prec(prec)
    out = np.zeros(B * HW * C + VAE_TAIL, dt)
    part = np.zeros(B * ((HW + 255) // 256) * 64 + B * 64 + VAE_TAIL, F32)
    c.check(c.lib.dd_dev_groupnorm(c.handle, code, B, HW, C, int(swish), P(np.ascontiguousarray(x, F32)), P(gamma), P(beta), P(out), P(part), None))
    return out, part


def run_softmax(prec, rows, n, scale, s):
    c = ctx()
    code, dt = _prec(prec)
    out = np.zeros(rows * n + VAE_TAIL, dt)
    c.check(c.lib.dd_dev_softmax_rows(c.handle, code, rows, n, float(scale), P(np.ascontiguousarray(s, F32)), P(out), None))
    return out


def values(out, prec):
    """the fp32 values of an output buffer (bf16 bits or fp32)"""
    return from_bf16_bits(out) if prec == "bf16" else out


# ---------------------------------------------------------------------------------------------------------------- the early-exit probes
# What tests/test_ee_probes.py (GPU, through dd_dev_ee_probe / dd_dev_ee_probe_reduce / dd_dev_ee_attn_probe) compares the probe kernels of
# csrc/rowops.hip with: float64 restatements from the fp32 operands with derived elementwise bounds, the reduce kernel in float32 in its
# fixed order, float32 restatements of the row and attention probes, and the inputs of every case.  `mutant` switches on one deliberate
# error; tests/test_kernel_support.py proves on the CPU that the inputs used on the GPU see each of them.
EE_TAIL = 64                   # DD_DEV_EE_TAIL: canary elements behind every output
EE_B = 3
EE_PROBE_L = (1, 5, 8, 9, 17, 65, 66, 257, 258)
EE_PROBE_CASES = [(512, L) for L in EE_PROBE_L] + [(D, L) for D in (64, 256, 768, 1024) for L in (17, 257)]      # (D, L)
EE_REDUCE_ROWS = (1, 3, 4, 5, 91)
EE_REDUCE_L = (1, 63, 64, 65, 257)
EE_ATTN_CASES = [(64, 2), (64, 17), (256, 65), (512, 257), (512, 258), (768, 257), (1024, 258)]                    # (D, L)
EE_ROW_MUTANTS = ("drop_slice_end", "pair_repeats", "no_bias")      # + "wrong_probe_row", which needs a table
EE_MEAN_MUTANTS = ("drop_tail", "over_patches")
EE_ATTN_MUTANTS = ("keep_first_token", "no_scale", "v_from_k", "w0_untransposed", "no_bv", "drop_far_tokens")
EE_PLANTED = (-120.0, 95.0, -88.9, 88.2, -95.0, 120.0, -90.0, -100.0)      # logits (before the bias) of the planted rows
FLOOR = 2.0 ** -126            # a result below the smallest normal fp32 may be flushed


def ee_probe_case(B, L, D, n_probe=1, row=0):
    """x [B, L, D], the probe table pw [n_probe, D] / pb [n_probe] (every row but `row` NaN), w = pw[row], b = pb[row].
    w ~ N(0, 1) / sqrt(D), shifted so that sum(w) = 0.02; b = 0.7.  Token row l of image b is of kind (l + b) % 4: N(0, 1) (logits within a
    few units); 30 N(0, 1) (logits of +-30); a multiple of w that plants the logit EE_PLANTED[(l // 4 + b) % 8] (saturation either way, expf
    overflow, results below 2^-126); 100 + N(0, 1) (a common offset of 100 sigma: sum |w| |x| = 80 sqrt(D) against a logit near 2 + b)"""
    r = np.random.default_rng(100000 * D + 100 * L + B + 7 * row)
    w = r.standard_normal(D) / np.sqrt(D)
    w = (w + (0.02 - w.sum()) / D).astype(F32)
    x = r.standard_normal((B, L, D))
    w64 = w.astype(np.float64)
    for b in range(B):
        for l in range(L):
            k = (l + b) % 4
            if k == 1:
                x[b, l] *= 30.0
            elif k == 2:
                x[b, l] = EE_PLANTED[(l // 4 + b) % 8] * w64 / (w64 @ w64) + 0.01 * x[b, l]
            elif k == 3:
                x[b, l] += 100.0
    pw = np.full((n_probe, D), np.nan, F32)
    pb = np.full(n_probe, np.nan, F32)
    pw[row], pb[row] = w, F32(0.7)
    return dict(B=B, L=L, D=D, x=x.astype(F32), pw=pw, pb=pb, w=w, b=F32(0.7))


def ee_slices(L):
    """the (l0, l1) row ranges of ee_probe_rows_kernel's 8 slices (the empty ones left out)"""
    per = -(-L // 8)
    return [(y * per, min(y * per + per, L)) for y in range(8) if y * per < L]


def _ee_row_mutation(s, mutant):
    """the row mutants, on s [B, L]: "drop_slice_end" -- the last row of each 8th-of-L slice keeps a stale value (the row's before it; the
    image's first row: 0); "pair_repeats" -- the second row in flight, l + 4, gets row l's value"""
    s = s.copy()
    L = s.shape[-1]
    if mutant == "drop_slice_end":
        src = s.copy()
        for _, l1 in ee_slices(L):
            s[:, l1 - 1] = src[:, l1 - 2] if l1 >= 2 else 0.0
    elif mutant == "pair_repeats":
        for l0, l1 in ee_slices(L):
            for l in range(l0, l1):
                if (l - l0) % 8 < 4 and l + 4 < l1:
                    s[:, l + 4] = s[:, l]
    return s


def probe_rows_ref(x, w, b, mutant=None, row=0, wrong_row=0):
    """(s, tol_s) [B, L]: s = sigmoid(x . w + b) in float64 from the fp32 operands; w [D] and b, or the probe table [n, D] / [n] and `row`.
    Derivation (u = 2^-24).  The kernel's logit is a per-lane fmaf chain of D / 64 terms, six xor-shuffle levels and the bias add, one
    rounding each (+ 1 spare): |da| <= (D / 64 + 6 + 2) u (|b| + sum |w| |x|).  It enters s with slope s (1 - s).  e = expf(-a) is allowed
    4 ulp, and its argument's own rounding is u |a|: relative error (4 + |a|) u of e, which enters s = 1 / (1 + e) as s (1 - s) (4 + |a|) u.
    The add and the divide round once each: 2 u s.  Second order: x 1.01.  An s below 2^-126 (a < -87.3; expf overflows from 88.7, then
    s = 0) may be flushed: + 2^-126.
    mutant: "drop_slice_end", "pair_repeats" (_ee_row_mutation), "no_bias", "wrong_probe_row" (table row `wrong_row` instead of `row`)"""
    w, b = np.asarray(w, np.float64), np.asarray(b, np.float64)
    if w.ndim == 2:
        pick = wrong_row if mutant == "wrong_probe_row" else row
        wm, bm, w, b = w[pick], b[pick], w[row], b[row]
    else:
        wm, bm = w, b
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        a = x @ w + b
        am = x @ wm + (0.0 if mutant == "no_bias" else bm)
        s, sm = 1.0 / (1.0 + np.exp(-a)), 1.0 / (1.0 + np.exp(-am))
    D = x.shape[-1]
    tol_a = (D / 64 + 6 + 2) * U24 * (np.abs(b) + np.abs(x) @ np.abs(w))
    tol = 1.01 * (s * (1 - s) * (tol_a + (4 + np.abs(a)) * U24) + 2 * U24 * s) + FLOOR
    return _ee_row_mutation(sm, mutant), tol


def probe_rows_f32(x, w, b):
    """ee_probe_rows_kernel in float32, in its own order: lane i's fmaf chain over k = i, i + 64, ..., the xor-shuffle tree, the bias, the
    sigmoid (numpy's float32 exp in expf's place; an fmaf as the float64 sum rounded once)"""
    x, w = np.asarray(x, F32), np.asarray(w, F32)
    D = x.shape[-1]
    acc = np.zeros(x.shape[:-1] + (64,), F32)
    for j in range(D // 64):
        acc = (acc.astype(np.float64) + x[..., 64 * j:64 * j + 64].astype(np.float64) * w[64 * j:64 * j + 64].astype(np.float64)).astype(F32)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., np.arange(64) ^ o]
    with np.errstate(over="ignore"):
        return F32(1.0) / (F32(1.0) + np.exp(-(acc[..., 0] + F32(b))))


def probe_mean_ref(s, tol_s=None, mutant=None):
    """(out, tol) [rows]: the mean over the last dimension of s in float64.  Derivation: lane i adds its ceil(L / 64) rows, six shuffle
    levels and one division follow, one rounding each; the terms are positive, so nothing cancels and the relative error is at most
    (ceil(L / 64) + 6 + 1) u (x 1.01, + 2^-126).  tol_s: the bound of the rows where s is their float64 reference and not the kernel's own
    fp32 rows -- the mean inherits its mean.
    mutant: "drop_tail" (the rows behind the last whole 64 left out of the sum), "over_patches" (the sum divided by L - 1)"""
    s = np.asarray(s, np.float64)
    L = s.shape[-1]
    out = s.mean(-1)
    tol = 1.01 * (-(-L // 64) + 6 + 1) * U24 * out + FLOOR + (0.0 if tol_s is None else np.asarray(tol_s).mean(-1))
    if mutant == "drop_tail":
        return s[..., :L // 64 * 64].sum(-1) / L, tol
    if mutant == "over_patches":
        with np.errstate(divide="ignore", invalid="ignore"):
            return s.sum(-1) / (L - 1), tol
    return out, tol


def probe_mean_f32(s):
    """ee_probe_reduce_kernel in float32 in its fixed order, bit for bit: lane i adds rows i, i + 64, ... ascending from 0, the xor-shuffle
    tree 32 .. 1, one division by (float)L.  s [rows, L] fp32 -> [rows] fp32"""
    s = np.asarray(s, F32)
    rows, L = s.shape
    pad = np.zeros((rows, round_up(L, 64)), F32)      # (a lane past the end adds nothing: + 0 is exact)
    pad[:, :L] = s
    acc = np.zeros((rows, 64), F32)
    for j in range(pad.shape[1] // 64):
        acc = acc + pad[:, 64 * j:64 * j + 64]
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, np.arange(64) ^ o]
    return acc[:, 0] / F32(L)


def ee_reduce_rows(rows, L):
    """srow [rows, L] fp32 for the reduce alone: sigmoid-like values in (0, 1) across 30 decades, with exact 0 and 1 among them"""
    r = np.random.default_rng(1000 * rows + L)
    s = r.uniform(0.0, 1.0, (rows, L)) * 10.0 ** -r.integers(0, 31, (rows, L)) * (r.uniform(size=(rows, L)) < 0.5)
    s = np.where(r.uniform(size=(rows, L)) < 0.3, r.uniform(0.0, 1.0, (rows, L)), s)
    s[::2, ::7] = 1.0
    s[:, L // 2] = 0.37
    s[:, L - 1] = 0.61      # (the last row: what a dropped tail drops)
    return s.astype(F32)


def _sparse_rows(r, rows, cols, nnz=4):
    """[rows, cols] with nnz entries N(0, 1) / 2 per row at random columns: |W v| is about |v| and sum |W| |v| is within 1.3 of it"""
    w = np.zeros((rows, cols))
    idx = np.argsort(r.random((rows, cols)), axis=1)[:, :nnz]
    w[np.arange(rows)[:, None], idx] = r.standard_normal((rows, nnz)) / 2.0
    return w


def ee_attn_case(B, L, D):
    """x [B, L, D] and an AttentionProbe's raw parameters.  q ~ 3 N(0, 1) and Wk ~ N(0, 1) / sqrt(D), dense, so the scores of N(0, 1) tokens
    have std about 3 and a few tokens share the softmax; bk ~ 5 N(0, 1) (the constant bk . q / sqrt(D) the fold drops), bv ~ N(0, 1).
    Wv and classification.0 hold four entries per row at random columns and classification.2 is positive: a bound carried elementwise
    through a dense Gaussian matrix grows by sqrt(2 D / pi) per stage over the error a kernel makes (5800 over the three stages at D = 512:
    no mutant below a relative error of 1 would show); through these it grows by 1.3, and a wrong index, row or transposition still hits
    other values.  With g = u / |u|^2 (u = Wk^T q / sqrt(D): adding c g to a token adds c to its score): token 0 of every image scores
    30 above the largest of the image's other tokens; the last token scores 0.5 below that (the tokens behind index 256 carry weight where
    there are any); in image 1 it scores 120 above (a single dominant token: every other probability underflows); every token of image 2 carries a
    common offset of 1000"""
    r = np.random.default_rng(100000 * D + 100 * L + B)
    q = (3.0 * r.standard_normal(D)).astype(F32)
    wkv = np.concatenate([r.standard_normal((D, D)) / np.sqrt(D), _sparse_rows(r, D, D)]).astype(F32)
    bkv = np.concatenate([5.0 * r.standard_normal(D), r.standard_normal(D)]).astype(F32)
    w0 = _sparse_rows(r, D, D).astype(F32)
    b0 = (0.5 * r.standard_normal(D)).astype(F32)
    w2 = (r.uniform(0.5, 1.5, D) * 4.0 / D).astype(F32)
    b2 = np.asarray([0.3], F32)
    u = wkv[:D].astype(np.float64).T @ q.astype(np.float64) / np.sqrt(D)
    g = u / (u @ u)
    x = r.standard_normal((B, L, D))
    for b in range(B):
        sc = x[b] @ u
        top = sc[1:max(L - 1, 2)].max()                                # the bulk's largest score
        x[b, L - 1] += (top + (120.0 if b % 3 == 1 else -0.5) - sc[L - 1]) * g
        x[b, 0] += (top + 30.0 - sc[0]) * g
        if b % 3 == 2:
            x[b] += 1000.0 * g
    return dict(B=B, L=L, D=D, x=x.astype(F32), q=q, wkv=wkv, bkv=bkv, w0=w0, b0=b0, w2=w2, b2=b2)


def attn_probe_ref(x, q, wkv, bkv, w0, b0, w2, b2, mutant=None):
    """(out, tol) [B]: AttentionProbe in float64 from the RAW fp32 parameters: tokens 1: only, k = Wk x + bk, score = q . k / sqrt(D),
    p = softmax(score), o = Wv sum_l p_l x_l + bv (= sum_l p_l v_l), out = w2 . silu(W0 o + b0) + b2.
    The bound, carried elementwise through the kernel's stages (u = 2^-24, n = L - 1 tokens, each stage x 1.01 for its second order):
    scores -- the kernel's are uf . x with uf = fl(Wk^T q / sqrt(D)) (one rounding each, the fold's sum is in double), a per-lane fmaf
      chain of D / 64 terms and six shuffle levels; they differ from the reference's by the constant bk . q / sqrt(D), which the softmax
      cancels, and by at most tsc_l = (1 + D / 64 + 6) u sum_k |uf_k| |x_lk|.
    softmax, as softmax_ref -- d_l = fl(sc_l - mx) rounds once, u |sc_l - sc_max| (a difference: the constant is not in it); expf is
      allowed 4 ulp: e_l has relative error R_l = tsc_l + (|sc_l - sc_max| + 4) u (a common shift of all scores, mx's own error, cancels).
      The sum adds ceil(n / 256) terms per thread, then the two-level block reduce (six shuffle levels, two adds across the four waves),
      T = ceil(n / 256) + 8 roundings, and inherits sum_l p_l R_l; 1 / sum rounds once.
    xbar_k = (chain of n fmaf of e_l x_lk) / sum: each term passes at most n roundings, the product with 1 / sum one more:
      txbar_k = sum_l p_l |x_lk| (R_l + sum_j p_j R_j + (n + T + 2) u) + 2^-126 sum_l |x_lk| (an e_l below 2^-126 may be flushed; sum >= 1).
    o = Wv xbar + bv and h = W0 o + b0 -- fmaf chains of D terms started on the bias (fma_chain64): (D + 3) u (|bias| + sum |W| |v|), plus
      the operand's bound through |W|.
    SiLU -- act = h / (1 + expf(-h)): slope <= 1.1 on h's bound; its own arithmetic (expf 4 ulp weighted 1 - sigmoid <= 1, the add, the
      divide) 6 u |act|; + 2^-126 (1 + |h|) where expf overflows.
    out -- per thread an fmaf chain of ceil(D / 256) terms, the block reduce's 8 roundings: (ceil(D / 256) + 8) u sum |w2| |act|; the add of
      b2 rounds the result itself, u |out|; and the bound of act through |w2|.
    mutant: "keep_first_token", "no_scale", "v_from_k" (rows 0 .. D-1 of weight_kv as Wv), "w0_untransposed", "no_bv", "drop_far_tokens"
    (the tokens behind index 256 left out of the softmax)"""
    x, q, wkv, bkv, w0, b0, w2, b2 = (np.asarray(a, np.float64) for a in (x, q, wkv, bkv, w0, b0, w2, b2))
    D = x.shape[-1]
    xs = x if mutant == "keep_first_token" else x[:, 1:]
    if mutant == "drop_far_tokens":
        xs = x[:, 1:257]
    n = xs.shape[1]
    wk, bk = wkv[:D], bkv[:D]
    wv = wk if mutant == "v_from_k" else wkv[D:]
    bv = np.zeros(D) if mutant == "no_bv" else bkv[D:]
    w0 = w0.T if mutant == "w0_untransposed" else w0
    sc = (xs @ wk.T + bk) @ q / (1.0 if mutant == "no_scale" else np.sqrt(D))
    d = sc - sc.max(-1, keepdims=True)
    e = np.exp(d)
    p = e / e.sum(-1, keepdims=True)
    ax = np.abs(xs)
    xbar = np.einsum("bl,blk->bk", p, xs)
    o = xbar @ wv.T + bv
    h = o @ w0.T + b0
    with np.errstate(over="ignore"):
        act = h / (1.0 + np.exp(-h))
    out = act @ w2.reshape(-1) + b2.reshape(-1)[0]
    # ---- the bound
    uf = np.abs(wk.T @ q / np.sqrt(D))
    tsc = (1 + D / 64 + 6) * U24 * (ax @ uf)
    R = 1.01 * (tsc + (np.abs(d) + 4) * U24)
    T = -(-n // 256) + 8
    pr = (p * R).sum(-1, keepdims=True)
    txbar = 1.01 * np.einsum("bl,blk->bk", p * (R + pr + (n + T + 2) * U24), ax) + FLOOR * ax.sum(1)
    to = 1.01 * ((D + 3) * U24 * (np.abs(bv) + np.abs(xbar) @ np.abs(wv).T) + txbar @ np.abs(wv).T)
    th = 1.01 * ((D + 3) * U24 * (np.abs(b0) + np.abs(o) @ np.abs(w0).T) + to @ np.abs(w0).T)
    tact = 1.01 * (1.1 * th + 6 * U24 * np.abs(act)) + FLOOR * (1 + np.abs(h))
    aw2 = np.abs(w2.reshape(-1))
    tol = 1.01 * ((-(-D // 256) + 8) * U24 * (np.abs(act) @ aw2) + U24 * np.abs(out) + tact @ aw2)
    return out, tol


def attn_probe_f32(x, q, wkv, bkv, w0, b0, w2, b2):
    """the folded form ee_attn_probe_kernel computes (u = Wk^T q / sqrt(D) in double, rounded once; no bk), evaluated in float32"""
    x, q64, wkv, bkv, w0, b0, w2, b2 = (np.asarray(a, F32) for a in (x, q, wkv, bkv, w0, b0, w2, b2))
    D = x.shape[-1]
    u = (wkv[:D].astype(np.float64).T @ q64.astype(np.float64) / np.sqrt(D)).astype(F32)
    xs = x[:, 1:]
    sc = xs @ u
    e = np.exp(sc - sc.max(-1, keepdims=True))
    inv = F32(1.0) / e.sum(-1, keepdims=True, dtype=F32)
    xbar = np.einsum("bl,blk->bk", e, xs).astype(F32) * inv
    o = xbar @ wkv[D:].T + bkv[D:]
    h = o @ w0.T + b0
    with np.errstate(over="ignore"):
        act = h / (F32(1.0) + np.exp(-h))
    return act @ w2.reshape(-1) + b2.reshape(-1)[0]


# ---- the GPU calls (tests marked gpu only)
def run_ee_probe(case, t_state=0, t_mul=0, add=0, reduce=True):
    """dd_dev_ee_probe -> (srow [B L + TAIL], out [B + TAIL] or None: the rows-only form)"""
    c = ctx()
    B, L, D = case["B"], case["L"], case["D"]
    srow = np.zeros(B * L + EE_TAIL, F32)
    out = np.zeros(B + EE_TAIL, F32) if reduce else None
    c.check(c.lib.dd_dev_ee_probe(c.handle, B, L, D, case["pw"].shape[0], t_state, t_mul, add, P(case["x"]), P(case["pw"]), P(case["pb"]),
                                  P(srow), P(out), None))
    return srow, out


def run_ee_reduce(s):
    c = ctx()
    s = np.ascontiguousarray(s, F32)
    out = np.zeros(s.shape[0] + EE_TAIL, F32)
    c.check(c.lib.dd_dev_ee_probe_reduce(c.handle, s.shape[0], s.shape[1], P(s), P(out), None))
    return out


def run_ee_attn(case, images=None):
    """dd_dev_ee_attn_probe on the case's images (all, or the slice `images`) -> out [B + TAIL]"""
    c = ctx()
    x = np.ascontiguousarray(case["x"] if images is None else case["x"][images])
    out = np.zeros(x.shape[0] + EE_TAIL, F32)
    c.check(c.lib.dd_dev_ee_attn_probe(c.handle, x.shape[0], case["L"], case["D"], P(x), *(P(case[k]) for k in ("q", "wkv", "bkv", "w0", "b0", "w2", "b2")),
                                       P(out), None))
    return out
