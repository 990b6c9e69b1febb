"""GPU unit tests of the GEMM path (csrc/gemm.hip gemm256_kernel / gemm_kernel, csrc/rowops.hip reduce_ln_kernel, csrc/rowlin.hip
rowlin768_kernel + csrc/mlp_fused.hip mlp_reduce_kernel) through their development entry points dd_dev_gemm / dd_dev_rowlin
(include/duodiff_dev.h), against float64 references built from the SAME bf16-rounded operands (as tests/test_qkv_attention.py does).

The gates are elementwise, not rms: a wrong 8-row LDS-DMA piece, a tail row that reads the wrong k chunk or a bias taken from the wrong
slot moves single elements by far more than fp32 accumulation does, and an rms over a whole model hides them.
  * fp32 results (x, split-K slabs):  |got - ref| <= 2^-16 (|A| . |W|^T + |bias| + |x_in|)
  * bf16 results: one bf16 ulp of bf16(ref) + the fp32 term (GELU: + the polynomial's error, gemm.hip gelu_erf4)
  * fp32 parity mode: 2^-20 of the same sum
  * LayerNorm (the oracle's, eps 1e-5) of the kernel's OWN fp32 rows: one bf16 ulp + 2^-16 of the rows' scale in units of their spread
test_gates_reject_the_bugs_they_are_meant_to_catch (CPU, no GPU mark) shows that the gates reject three such bugs.
Every output buffer comes back whole with its canary space (rows up to round_up(M, 256) + 8, columns up to ldo, the head-major padding rows,
the slab area past M N splits): bytes outside the contract must still hold the canary.
"""
import ctypes as C

import numpy as np
import pytest

import kernel_support
from kernel_support import (FP32_REL, GELU_POLY, GELU_SLOPE, NAN32, PARITY_REL, PREC_BF16, PREC_FP32, P, bf16, from_bf16_bits, gate, gelu_exact,
                            ln_ref_and_tol, round_up, unfrag, untouched, ulp_bf16)

gpu = pytest.mark.gpu

EPI_STORE, EPI_BIAS_GELU, EPI_BIAS_RESID, EPI_BIAS_SET, EPI_BIAS_STORE = range(5)
EPI_NAME = {EPI_STORE: "store", EPI_BIAS_GELU: "bias_gelu", EPI_BIAS_RESID: "bias_resid", EPI_BIAS_SET: "bias_set", EPI_BIAS_STORE: "bias_store"}


# ---------------------------------------------------------------------------------------------------------------- operands
def operands(M, N, K, seed, bias_span=None, x_offset=0.0):
    r = np.random.default_rng(seed)
    A = r.standard_normal((M, K), dtype=np.float32)
    W = (r.standard_normal((N, K), dtype=np.float32) / np.sqrt(K)).astype(np.float32)
    if bias_span:      # pre-activations over +-bias_span: the whole range of the GELU polynomial and its clamp
        bias = r.permutation(np.linspace(-bias_span, bias_span, N)).astype(np.float32)
    else:
        bias = (0.5 * r.standard_normal(N)).astype(np.float32)
    x = (r.standard_normal((M, N)) + x_offset).astype(np.float32)
    return A, W, bias, x


def linear_ref(A, W, prec=PREC_BF16, k0=0, k1=None):
    """float64 A[:, k0:k1] . W[:, k0:k1]^T of the operands the kernel sees, and |A| . |W|^T of the same"""
    q = bf16 if prec == PREC_BF16 else (lambda a: a)
    a = q(A[:, k0:k1]).astype(np.float64)
    w = q(W[:, k0:k1]).astype(np.float64)
    return a @ w.T, np.abs(a) @ np.abs(w).T


# ---------------------------------------------------------------------------------------------------------------- GPU calls
def run_gemm(A, W, bias, x_in, epi, K1=0, prec=PREC_BF16, tile128=-1, hm=None, splits=0, resid=1, ln=None, tok=(0, 0), frag=False,
             ldo=None, with_out=True, num_cus=0):
    """dd_dev_gemm; returns (xres [Mo, N], out, h, frag, slabs) as the whole buffers"""
    ctx = kernel_support.ctx()
    M, K = A.shape
    N = W.shape[0]
    K1 = K1 or K
    Mo = round_up(M, 256) + 8
    ldo = ldo or N
    a1 = np.ascontiguousarray(A[:, :K1])
    a2 = np.ascontiguousarray(A[:, K1:]) if K1 < K else None
    xres = np.full((Mo, N), NAN32, np.uint32).view(np.float32)
    if x_in is not None:
        xres[:M] = x_in
    L, H = hm if hm else (0, 0)
    if hm:
        Lp = round_up(L, 8)
        out = np.zeros((M // L * 3 * H * Lp + 64) * 64, np.uint16 if prec == PREC_BF16 else np.float32)
    else:
        out = np.zeros((Mo, ldo), np.uint16 if prec == PREC_BF16 else np.float32)
    out = out if with_out else None
    h = np.zeros((Mo, N), np.uint16) if ln is not None else None
    fr = np.zeros((Mo, N), np.uint16) if frag else None
    slab = np.zeros((max(splits, 0), Mo, N), np.float32) if splits else None
    lnp = None if ln is None else np.ascontiguousarray(np.stack(ln), np.float32)
    ctx.check(ctx.lib.dd_dev_gemm(ctx.handle, prec, M, N, K, K1, P(a1), P(a2), P(np.ascontiguousarray(W)), P(bias), epi, tile128, L, H, splits,
                                  resid, P(lnp), tok[0], tok[1], P(xres), P(out), ldo, P(h), P(fr), P(slab), num_cus, 0, None, C.byref(C.c_float(0))))
    return xres, out, h, fr, slab


def run_rowlin(A, W, bias, x_in, B, n_patches, extras, k_split=0, set_x=0, ln=None, frag=False, copy=True):
    ctx = kernel_support.ctx()
    M, K = A.shape
    Mo = round_up(M, 256) + 8
    a1 = np.ascontiguousarray(A[:, :k_split] if k_split else A)
    a2 = np.ascontiguousarray(A[:, k_split:]) if k_split else None
    xres = np.full((Mo, 768), NAN32, np.uint32).view(np.float32)
    xres[:M] = x_in
    xc = np.zeros((Mo, 768), np.uint16) if copy else None
    h = np.zeros((Mo, 768), np.uint16) if ln is not None else None
    lnp = None if ln is None else np.ascontiguousarray(np.stack(ln), np.float32)
    ctx.check(ctx.lib.dd_dev_rowlin(ctx.handle, B if n_patches else M, n_patches, extras, K, k_split, set_x, P(a1), P(a2),
                                    P(np.ascontiguousarray(W)), P(bias), P(lnp), P(xres), P(xc), P(h), 1 if frag else 0, 0, None,
                                    C.byref(C.c_float(0))))
    return xres, xc, h


def ln_params(D, seed):
    r = np.random.default_rng(seed)
    return (1.0 + 0.3 * r.standard_normal(D)).astype(np.float32), (0.2 * r.standard_normal(D)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- checks
def check_linear(name, M, N, K, epi, K1=0, prec=PREC_BF16, tile128=-1, ldo=None, seed=0, with_out=True, num_cus=0, ops=None, rel=None,
                 report=None):
    """one launch under the gates of the module docstring.  ops: the caller's (A, W, bias, x_in) instead of operands(seed) -- bias None
    (EPI_STORE, or EPI_BIAS_SET without a bias): the launch gets a null bias and the reference adds none; x_in None: x holds canary bytes
    before the launch.  rel: the factor of the fp32 term where the caller has derived one for its class of operands (tests/test_vae_gemm.py);
    None: FP32_REL / PARITY_REL.  report: a dict that receives the largest error / bound ratios"""
    span = 12.0 if epi == EPI_BIAS_GELU else None
    A, W, bias, x_in = ops if ops is not None else operands(M, N, K, seed, bias_span=span)
    assert A.shape == (M, K) and W.shape == (N, K) and (bias is not None or epi in (EPI_STORE, EPI_BIAS_SET))
    xres, out, _, _, _ = run_gemm(A, W, bias, x_in, epi, K1=K1, prec=prec, tile128=tile128, ldo=ldo, with_out=with_out, num_cus=num_cus)
    acc, absum = linear_ref(A, W, prec)
    rel = rel if rel is not None else FP32_REL if prec == PREC_BF16 else PARITY_REL
    b64 = bias.astype(np.float64) if bias is not None else np.zeros(N)
    if x_in is None:
        assert epi != EPI_BIAS_RESID
        x_in = np.full((M, N), NAN32, np.uint32).view(np.float32)      # (the canary bytes run_gemm fills x with: an epilogue that does not write x leaves them)
    pre = acc + (b64 if epi != EPI_STORE else 0.0)
    t32 = rel * (absum + (np.abs(b64) if epi != EPI_STORE else 0.0))
    ratios = {}
    if epi in (EPI_BIAS_RESID, EPI_BIAS_SET):
        xref = pre + (x_in.astype(np.float64) if epi == EPI_BIAS_RESID else 0.0)
        tx = t32 + (rel * np.abs(x_in) if epi == EPI_BIAS_RESID else 0.0)
        ratios["x"] = gate(xres[:M], xref, tx, f"{name}: x")
        oref, tout = xref, tx
    else:
        assert np.array_equal(xres[:M].view(np.uint32), np.ascontiguousarray(x_in, np.float32).view(np.uint32)), f"{name}: x written by an epilogue that does not write it"
        if epi == EPI_BIAS_GELU:
            oref = gelu_exact(pre)
            tout = GELU_SLOPE * t32 + (GELU_POLY + 2.0 ** -22 * np.abs(pre) if prec == PREC_BF16 else 4 * 2.0 ** -24 * np.abs(oref))
        else:
            oref, tout = pre, t32
    assert untouched(xres[M:]), f"{name}: x rows >= M written"
    if out is not None and epi != EPI_BIAS_SET:
        if prec == PREC_BF16:
            got = from_bf16_bits(out[:M, :N])
            ratios["out"] = gate(got, oref, ulp_bf16(oref) + tout, f"{name}: out")
            assert untouched(out[M:]) and untouched(out[:, N:]), f"{name}: out written outside [M, N)"
        else:
            ratios["out"] = gate(out[:M, :N], oref, tout + 1e-30, f"{name}: out")
            assert untouched(out[M:]) and untouched(out[:, N:]), f"{name}: out written outside [M, N)"
    elif out is not None:
        assert untouched(out), f"{name}: EPI_BIAS_SET wrote out"
    print(f"{name}: M={M} N={N} K={K} K1={K1 or K} {EPI_NAME[epi]} tile128={tile128} ldo={ldo or N}: max err/bound "
          + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    if report is not None:
        report.update(ratios)
    return xres, out


# gemm256 (tile128 = 0: the persistent 256 x 256 kernel), every epilogue, every row partition the model meets: M = 256 q + e q
# (e = 0 .. 8 tail rows per tile; 264 = one tile + 8; 528 = 2 tiles + 8 each; 2112 = 8 tiles + 8 each), skip_linear's concat
GEMM256 = [
    (256, 512, 512, 0, EPI_BIAS_RESID),
    (257, 768, 768, 0, EPI_BIAS_GELU),
    (264, 1024, 64, 0, EPI_STORE),
    (528, 1536, 512, 0, EPI_BIAS_STORE),
    (2112, 768, 768, 0, EPI_BIAS_RESID),
    (774, 3072, 512, 0, EPI_BIAS_GELU),
    (1285, 512, 3072, 0, EPI_BIAS_RESID),
    (774, 768, 1536, 768, EPI_BIAS_SET),
    (1285, 1024, 2048, 1024, EPI_BIAS_SET),
    (514, 1024, 1024, 0, EPI_BIAS_STORE),
    (771, 1536, 512, 0, EPI_STORE),
]


@gpu
@pytest.mark.parametrize("M,N,K,K1,epi", GEMM256)
def test_gemm256_against_float64_reference(M, N, K, K1, epi):
    lib = kernel_support.ctx().lib
    q, e = C.c_int(), C.c_int()
    if lib.dd_plan_rows(M, N, K, 256, C.byref(q), C.byref(e)) == 0:
        print(f"  plan256 at 256 CUs: q={q.value} e={e.value}")
    check_linear("gemm256", M, N, K, epi, K1=K1, tile128=0, ldo=N + 64 if epi == EPI_BIAS_RESID else None, seed=M + N + K)


@gpu
@pytest.mark.parametrize("M,N,K,epi", [(1285, 1024, 1024, EPI_BIAS_RESID), (774, 1536, 512, EPI_BIAS_GELU)])
def test_tile128_forced_either_way_on_one_shape(M, N, K, epi):
    """tile128 = 1 (the 128 x 128 kernel, ragged last M tile) and 0 (the persistent kernel) on the same shape: both pass the gate"""
    for t in (1, 0):
        check_linear(f"tile128={t}", M, N, K, epi, tile128=t, seed=7)


@gpu
@pytest.mark.parametrize("M,N,K,epi", [(300, 192, 512, EPI_BIAS_STORE), (100, 48, 256, EPI_BIAS_SET), (200, 512, 512, EPI_BIAS_GELU),
                                       (300, 512, 768, EPI_BIAS_RESID), (37, 256, 1024, EPI_STORE)])
def test_generic_128_kernel_against_float64_reference(M, N, K, epi):
    """shapes the 256 x 256 kernel does not take: N not a multiple of 256, M < 256, ragged M"""
    check_linear("gemm128", M, N, K, epi, seed=M * N, ldo=N + 8 if epi != EPI_BIAS_SET else None)


@gpu
@pytest.mark.parametrize("M,N,K,epi", [(300, 512, 256, EPI_BIAS_RESID), (300, 48, 512, EPI_BIAS_SET), (257, 256, 128, EPI_BIAS_GELU),
                                       (129, 64, 512, EPI_BIAS_STORE)])
def test_fp32_parity_kernels_against_float64_reference(M, N, K, epi):
    """gemm_kernel<float>: 128 x 128, and the 128 x 64 form for N <= 64 (decoder_pred); exact-erf GELU"""
    check_linear("gemm fp32", M, N, K, epi, prec=PREC_FP32, seed=M + K)


@gpu
@pytest.mark.parametrize("D,L,B,bias", [(512, 257, 3, True), (768, 258, 2, False), (1024, 257, 2, True), (512, 65, 2, False), (768, 257, 1, True)])
def test_head_major_qkv_store(D, L, B, bias):
    """attn.qkv written head-major: every (image, q|k|v head) unit is Lp = round_up(L, 8) rows of 64; rows [L, Lp) and the space behind the
    image keep their canary bytes (M = 130: the 128 x 128 kernel's head-major store)"""
    H, M, N = D // 64, B * L, 3 * D
    A, W, b, _ = operands(M, N, D, D + L)
    epi = EPI_BIAS_STORE if bias else EPI_STORE
    _, out, _, _, _ = run_gemm(A, W, b, None, epi, hm=(L, H))
    acc, absum = linear_ref(A, W)
    ref = acc + (b if bias else 0.0)
    tol = ulp_bf16(ref) + FP32_REL * (absum + (np.abs(b) if bias else 0.0))
    Lp = round_up(L, 8)
    img = out[: B * 3 * H * Lp * 64].reshape(B, 3 * H, Lp, 64)
    got = from_bf16_bits(img[:, :, :L, :]).transpose(0, 2, 1, 3).reshape(M, N)
    r = gate(got, ref, tol, "head-major qkv")
    assert untouched(img[:, :, L:, :]), "rows [L, Lp) of a head-major unit written"
    assert untouched(out[B * 3 * H * Lp * 64:]), "bytes behind the head-major image written"
    print(f"head-major D={D} L={L} B={B} bias={bias}: max err/bound {r:.3f}")


# split-K: (N = D, K, K1, splits, resid, LayerNorm, frag, images of L tokens, extras, x offset)
SPLITK = [
    (256, 1024, 0, 4, 1, True, True, 258, 2, 0.0),
    (256, 512, 0, 2, 0, False, False, 257, 1, 0.0),
    (512, 512, 0, 2, 1, True, False, 257, 3, 0.0),
    (512, 2048, 0, 4, 1, True, True, 257, 2, 100.0),
    (768, 1536, 768, 2, 0, True, True, 258, 2, 0.0),
    (768, 3072, 0, 4, 1, True, False, 258, 2, 0.0),
    (1024, 2048, 1024, 4, 0, False, False, 257, 2, 0.0),
    (1024, 1024, 0, 2, 1, True, False, 258, 2, 100.0),
    (1024, 4096, 0, 2, 1, True, True, 257, 1, 0.0),
]


def check_split_k(D, K, K1, splits, resid, with_ln, frag, L, B, x_offset, n_patches=256):
    """split-K + reduce_ln on B images of L tokens, the last n_patches of each its patch rows: the slabs against their k ranges, x, the bf16
    copy and the LayerNorm under the gates of the module docstring.  Returns the largest error / bound ratio of each"""
    M = B * L
    A, W, bias, x_in = operands(M, D, K, D + K + splits, x_offset=x_offset)
    ln = ln_params(D, D) if with_ln else None
    xres, out, h, fr, slab = run_gemm(A, W, bias, x_in, EPI_BIAS_RESID, K1=K1, splits=splits, resid=resid, ln=ln, tok=(L, L - n_patches), frag=frag)
    nk = K // 64
    ratios = {}
    for sp in range(splits):
        k0, k1 = sp * nk // splits * 64, (sp + 1) * nk // splits * 64
        acc, absum = linear_ref(A, W, k0=k0, k1=k1)
        ratios[f"slab {sp}"] = gate(slab.reshape(-1)[sp * M * D: (sp + 1) * M * D].reshape(M, D), acc, FP32_REL * absum, f"slab {sp}")     # (slab sp at sp M N)
    assert untouched(slab.reshape(-1)[splits * M * D:]), "slab area past M N splits written"
    acc, absum = linear_ref(A, W)
    xref = acc + bias + (x_in.astype(np.float64) if resid else 0.0)
    tx = FP32_REL * (absum + np.abs(bias) + (np.abs(x_in) if resid else 0.0))
    rx = gate(xres[:M], xref, tx, "x")
    assert untouched(xres[M:]), "x rows >= M written"
    ro = gate(from_bf16_bits(out[:M]), xref, ulp_bf16(xref) + tx, "bf16 copy")
    assert untouched(out[M:]), "copy rows >= M written"
    msg = f"split-K D={D} K={K} K1={K1 or K} splits={splits} resid={resid} ln={with_ln} frag={frag} L={L} B={B}: max err/bound x {rx:.3f}, copy {ro:.3f}"
    if with_ln:
        want, tol = ln_ref_and_tol(xres[:M], *ln)
        patch = (np.arange(M) % L) >= L - n_patches
        if frag:
            groups = B * n_patches // 32
            got_p = unfrag(fr.reshape(-1), groups, D)
            rh = gate(from_bf16_bits(got_p), want[patch], tol[patch], "LayerNorm (fragment order)")
            assert untouched(fr.reshape(-1)[groups * 32 * D:]), "fragment buffer written past the patch rows"
            rows = ~patch
            assert untouched(h[:M][patch]), "patch rows' LayerNorm written row-major too"
        else:
            rows = np.ones(M, bool)
        rh2 = gate(from_bf16_bits(h[:M][rows]), want[rows], tol[rows], "LayerNorm (row-major)")
        assert untouched(h[M:]), "LayerNorm rows >= M written"
        msg += f", LayerNorm row-major {rh2:.3f}" + (f", fragment order {rh:.3f}" if frag else "")
        ratios["LayerNorm"] = max(rh2, rh if frag else 0.0)
    print(msg)
    ratios.update(x=rx, copy=ro)
    return ratios


@gpu
@pytest.mark.parametrize("D,K,K1,splits,resid,with_ln,frag,L,B,x_offset", SPLITK)
def test_split_k_and_reduce_ln_against_float64_reference(D, K, K1, splits, resid, with_ln, frag, L, B, x_offset):
    """every reduce_ln_kernel<NQ> (D = 256 .. 1024), 2 and 4 slabs, residual or not, LayerNorm row-major or in fragment order (rows with a
    common offset of 100 sigma included); the slabs themselves against their k ranges"""
    check_split_k(D, K, K1, splits, resid, with_ln, frag, L, B, x_offset, n_patches=256)


# rowlin768: (B, patches, extras, K, k_split, set_x, frag, x_copy, LayerNorm, x offset)
ROWLIN = [
    (1, 64, 1, 768, 0, 0, False, True, True, 0.0),
    (3, 256, 2, 3072, 0, 0, True, True, True, 0.0),
    (5, 256, 1, 768, 0, 0, False, False, True, 0.0),
    (3, 64, 0, 1536, 768, 1, True, True, True, 0.0),
    (5, 64, 2, 1536, 768, 1, False, True, True, 0.0),
    (3, 256, 1, 3072, 0, 0, False, True, True, 100.0),
    (1, 256, 2, 3072, 0, 0, False, True, False, 0.0),
]


def check_rowlin(name, B, P_, E, K, k_split, set_x, frag, copy, with_ln, x_offset, M_plain=0, seed=0):
    M = B * (P_ + E) if P_ else M_plain
    A, W, bias, x_in = operands(M, 768, K, seed, x_offset=x_offset)
    ln = ln_params(768, K) if with_ln else None
    xres, xc, h = run_rowlin(A, W, bias, x_in, B, P_, E, k_split=k_split, set_x=set_x, ln=ln, frag=frag, copy=copy)
    acc, absum = linear_ref(A, W)
    xref = acc + bias + (0.0 if set_x else x_in.astype(np.float64))
    tx = FP32_REL * (absum + np.abs(bias) + (0.0 if set_x else np.abs(x_in)))
    rx = gate(xres[:M], xref, tx, f"{name}: x")
    assert untouched(xres[M:]), f"{name}: x rows >= M written"
    msg = f"{name} B={B} patches={P_} extras={E} M={M} K={K} k_split={k_split} set_x={set_x} frag={frag}: max err/bound x {rx:.3f}"
    if copy:
        msg += f", copy {gate(from_bf16_bits(xc[:M]), xref, ulp_bf16(xref) + tx, f'{name}: x copy'):.3f}"
        assert untouched(xc[M:]), f"{name}: copy rows >= M written"
    if with_ln:
        want, tol = ln_ref_and_tol(xres[:M], *ln)
        if frag:
            patch = (np.arange(M) % (P_ + E)) >= E if P_ else np.ones(M, bool)
            groups = int(patch.sum()) // 32
            got = unfrag(h.reshape(-1), groups, 768)
            msg += f", LayerNorm fragment order {gate(from_bf16_bits(got), want[patch], tol[patch], f'{name}: LayerNorm (fragment order)'):.3f}"
            assert untouched(h.reshape(-1)[groups * 32 * 768:]), f"{name}: fragment buffer written past the patch rows"
        else:
            msg += f", LayerNorm {gate(from_bf16_bits(h[:M]), want, tol, f'{name}: LayerNorm'):.3f}"
            assert untouched(h[M:]), f"{name}: LayerNorm rows >= M written"
    print(msg)
    return xres, xc, h


@gpu
@pytest.mark.parametrize("B,P_,E,K,k_split,set_x,frag,copy,with_ln,x_offset", ROWLIN)
def test_rowlin_against_float64_reference(B, P_, E, K, k_split, set_x, frag, copy, with_ln, x_offset):
    """main tiles (patch rows), the K-split extra-token tiles + mlp_reduce, skip_linear's concat with x = (no residual), both LayerNorm
    orders, rows with a common offset of 100 sigma"""
    check_rowlin("rowlin", B, P_, E, K, k_split, set_x, frag, copy, with_ln, x_offset, seed=B * K + E)


@gpu
@pytest.mark.parametrize("M,K,frag", [(300, 768, False), (200, 3072, False), (96, 1536, True)])
def test_rowlin_plain_mode(M, K, frag):
    """tok_n == 0: rows [0, M) in tiles of 128, a ragged last tile"""
    check_rowlin("rowlin plain", 1, 0, 0, K, 0, 0, frag, True, True, 0.0, M_plain=M, seed=M)


# ---------------------------------------------------------------------------------------------------------------- invariants, bit for bit
@gpu
@pytest.mark.parametrize("M,N,K,epi,splits", [(2112, 768, 768, EPI_BIAS_RESID, 0), (1285, 1536, 512, EPI_BIAS_GELU, 0), (774, 1024, 1024, EPI_BIAS_RESID, 2)])
def test_persistent_grid_size_does_not_change_a_bit(M, N, K, epi, splits):
    """num_cus 8 (every workgroup walks many tiles: the bias slot parity, the k-tile stream across tile boundaries), 64 and the device's"""
    A, W, bias, x_in = operands(M, N, K, 11, bias_span=12.0 if epi == EPI_BIAS_GELU else None)
    res = []
    for cus in (8, 64, 0):
        ln = ln_params(N, 3) if splits else None
        res.append(run_gemm(A, W, bias, x_in, epi, tile128=0, splits=splits, ln=ln, num_cus=cus))
    for other in res[1:]:
        for a, b in zip(res[0], other):
            if a is not None:
                assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
    if not splits:
        check_linear("gemm256 at 8 CUs", M, N, K, epi, tile128=0, num_cus=8, seed=5)
    print(f"num_cus 8 / 64 / device: identical bytes (M={M} N={N} K={K} splits={splits})")


@gpu
def test_last_rows_equal_a_smaller_call():
    """the last 2 images of a 5-image call equal a 2-image call of those rows (the row-level form of `two chains == one chain`): GEMM (the rows
    fall into main tiles of one call and tail rows of the other), split-K + reduce_ln, rowlin"""
    L, D = 257, 1024
    A, W, bias, x_in = operands(5 * L, D, D, 21)
    tail = slice(3 * L, 5 * L)
    for kw in (dict(epi=EPI_BIAS_RESID, tile128=0), dict(epi=EPI_BIAS_RESID, tile128=1), dict(epi=EPI_BIAS_RESID, splits=2, ln=ln_params(D, 1))):
        big = run_gemm(A, W, bias, x_in, **kw)
        small = run_gemm(A[tail], W, bias, x_in[tail], **kw)
        assert np.array_equal(big[0][tail].view(np.uint32), small[0][: 2 * L].view(np.uint32)), kw
        assert np.array_equal(big[1][tail], small[1][: 2 * L]), kw
        if kw.get("ln"):
            assert np.array_equal(big[2][tail], small[2][: 2 * L]), kw
    L = 258
    A, W, bias, x_in = operands(5 * L, 768, 3072, 22)
    tail = slice(3 * L, 5 * L)
    ln = ln_params(768, 2)
    big = run_rowlin(A, W, bias, x_in, 5, 256, 2, ln=ln)
    small = run_rowlin(A[tail], W, bias, x_in[tail], 2, 256, 2, ln=ln)
    for a, b in zip(big, small):
        assert np.array_equal(a[tail].view(np.uint8), b[: 2 * L].view(np.uint8))


# ---------------------------------------------------------------------------------------------------------------- the gates themselves (CPU)
def test_gates_reject_the_bugs_they_are_meant_to_catch():
    """The elementwise gates above, applied to three perturbed references, reject each: one 64-k chunk of one 8-row LDS-DMA piece dropped;
    one 256-column tile's bias shifted by one column; the two split-K slabs swapped with one of them scaled by 1 + 2^-10."""
    M, N, K = 264, 512, 512
    A, W, bias, x_in = operands(M, N, K, 1)
    acc, absum = linear_ref(A, W)
    xref = acc + bias + x_in
    tx = FP32_REL * (absum + np.abs(bias) + np.abs(x_in))
    # what a correct kernel returns: the reference rounded to fp32 passes, and so does its bf16 copy
    assert gate(xref.astype(np.float32), xref, tx, "fp32 of the reference") < 1.0
    assert gate(bf16(xref.astype(np.float32)), xref, ulp_bf16(xref) + tx, "bf16 of the reference") <= 1.0
    # 1: rows 8..15 (one LDS-DMA piece) without k 64..127
    bad = xref.copy()
    chunk, _ = linear_ref(A[8:16], W, k0=64, k1=128)
    bad[8:16] -= chunk
    with pytest.raises(AssertionError):
        gate(bad.astype(np.float32), xref, tx, "piece without one k chunk")
    with pytest.raises(AssertionError):
        gate(bf16(bad.astype(np.float32)), xref, ulp_bf16(xref) + tx, "bf16 copy of the same")
    # 2: column tile 1's bias one column off
    bad = xref.copy()
    bad[:, 256:512] += np.roll(bias, -1)[256:512] - bias[256:512]
    with pytest.raises(AssertionError):
        gate(bad.astype(np.float32), xref, tx, "bias shifted by one column")
    # 3: split-K slabs swapped, one of them scaled by 1 + 2^-10: the slabs' own gate and x's
    s0, a0 = linear_ref(A, W, k0=0, k1=256)
    s1, a1 = linear_ref(A, W, k0=256, k1=512)
    got0, got1 = (s1 * (1 + 2.0 ** -10)).astype(np.float32), s0.astype(np.float32)
    with pytest.raises(AssertionError):
        gate(got0, s0, FP32_REL * a0, "slab 0")
    with pytest.raises(AssertionError):
        gate((got0.astype(np.float64) + got1 + bias + x_in).astype(np.float32), xref, tx, "x from the swapped, scaled slabs")
    # the GELU bound of the bf16 mode: the polynomial of gemm.hip gelu_erf4 (fp32, on the CPU) stays within GELU_POLY over +-16
    v = np.linspace(-16, 16, 200001).astype(np.float32)
    f = np.float32
    sc = np.clip(v, f(-3.8), f(3.8))
    s2 = sc * sc
    p = s2 * f(7.331517960e-08) + f(-4.544908101e-06)
    for c in (1.213693460e-04, -1.863093246e-03, 1.863326334e-02, -1.314395642e-01, 7.973534865e-01):
        p = (p * s2 + f(c)).astype(np.float32)
    hv = v * f(0.5)
    poly = (hv * (p * sc) + hv).astype(np.float64)
    assert np.abs(poly - gelu_exact(v)).max() <= GELU_POLY
