"""Per-element float64 tests of every launch a long model (more than 288 tokens) makes besides attention, at long image
geometries, through the development entry points (include/duodiff_dev.h).  tests/test_attention_long.py gates the streaming attention kernel;
tests/test_long_sequence.py compares whole models with the oracle, the bf16 engine under an rms over the whole output, under which a fault
confined to one ragged row tile, one column tile of one image or one extra-token row can stay.  What a long model changes is address
arithmetic: tok_n / tok_e / tok_l in mlp_fused.hip and rowlin.hip, HeadMajor::Lp and its magic divide, pidx / lidx of the fused qkv phases, the
gy / gx patch grid of embed_kernel, the tile grid of final_tiled_kernel.

Operands, references, gates and run helpers are those of the per-kernel test files, imported; every tolerance is the imported gate's own formula
and no bound is introduced here.  Every output buffer comes back whole: canary rows behind M, the rows [L, Lp) of every head-major unit and the
space behind the image must still hold 0xFF.  Each GPU test prints its largest error / bound ratio on a line that starts with `long geometry`.

  family (entry point)                       cases
  head-major qkv store (dd_dev_gemm)         L = 289, 325, 578, 577, 1025, 4098: Lp - L = 7, 3, 6, 7, 7, 6 pad rows, row tiles straddling images;
                                             the 128 x 128 kernel, the fp32 parity kernel, and gemm256 at M = 1025 and 2050
  fused block tail (dd_dev_block_tail)       N = 324 (N % 32 = 4), 576 with two extra tokens, 1024: the launches of blocks 0, 1, 2 of a depth-3 model
  row-resident Linear (dd_dev_rowlin)        embed_dim 768 at tok_n = 576 / 1024: attn.proj, mlp.fc2, skip_linear
  split-K + reduce_ln (dd_dev_gemm)          embed_dim 1024 at L = 1025 (the model choose_paths gives split-K); the L = 577 model's GEMM sequence
  head_dec, patch-rows form                  36 and 64 sixteen-row units per image
  token assembly, generic kernel             grids 18, 24, 32 and 64 patches wide, 4096 patches
  time_mlp_kernel                            row extras - 1 of images of 325 / 4098 rows
  step tail (dd_dev_final)                   S = 72 (4.5 x 4.5 tiles), 96, 128 (8 x 8 tiles); one Philox DDPM step at S = 128, b0 > 0

The CPU tests (no GPU mark) apply the same gates to an emulation of the correct arithmetic, which must pass, and to emulations of the geometry
faults a long model can bring out, each of which must be rejected: a test of nothing fails itself.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import kernel_support as ks
from duodiff_amd import _lib
from kernel_support import (FP32_REL, NAN16, NAN32, PARITY_REL, PREC_BF16, PREC_FP32, F32, P, bf16_bits, from_bf16_bits, gate, round_up, untouched,
                            ulp_bf16)
from test_block_tail import check as tail_check
from test_block_tail import emulate as tail_emulate
from test_block_tail import ops_for, same_bytes
from test_block_tail import run as tail_run
from test_final_step import PHILOX_BOUND, Out, check_eps, combo, draw, ff, launch, run_step
from test_gemm_path import (EPI_BIAS_GELU, EPI_BIAS_RESID, EPI_BIAS_SET, EPI_BIAS_STORE, EPI_STORE, check_linear, check_rowlin, check_split_k,
                            linear_ref, operands, run_gemm)
from test_head_dec import HEAD_DEC_REL
from test_head_dec import _reference as head_reference
from test_head_dec import _run as head_run
from test_row_kernels import embed_operands, embed_ref, run_embed, time_mlp_operands, time_mlp_ref, time_mlp_tolerance

gpu = pytest.mark.gpu


def report(family, case, ratios):
    """the line the ratios of DESIGN section 7o are collected from"""
    worst = max(ratios.values()) if isinstance(ratios, dict) else float(ratios)
    print(f"long geometry | {family} | {case}: largest error / bound {worst:.3f}")
    return worst


def flat(ratios):
    """{gate: {row class: ratio}} of test_block_tail.check -> {gate row class: ratio}"""
    return {f"{k} {c}": v for k, d in ratios.items() for c, v in d.items()}


# ---------------------------------------------------------------------------------------------------------------- head-major qkv store
# (D, L, B).  Every row count but the last two's (1025 = 256 x 4 + 1, 2050 = 256 x 8 + 2) has no row partition of the 256 x 256 kernel and N = 384
# never has its column tiles: those cases run the 128 x 128 kernel whatever tile128 says; the last two run gemm256's head-major store
HM_CASES = [(128, 289, 3), (128, 325, 3), (512, 578, 2), (768, 577, 2), (1024, 577, 2), (128, 1025, 1), (128, 4098, 2), (512, 1025, 1),
            (1024, 1025, 2)]
HM_FP32 = [(128, 325, 3), (128, 4098, 2)]
HM_BIAS = (512, 578, 2)


@functools.lru_cache(maxsize=2)
def hm_case(D, L, B, bias, prec):
    """(A, W, b, ref, tol) of attn.qkv on B images of L tokens: the gate of test_gemm_path.test_head_major_qkv_store (bf16) and of its fp32 parity
    tests (check_linear)"""
    M, N = B * L, 3 * D
    A, W, b, _ = operands(M, N, D, D + L)
    acc, absum = linear_ref(A, W, prec)
    ref = acc + (b if bias else 0.0)
    mag = absum + (np.abs(b) if bias else 0.0)
    tol = ulp_bf16(ref) + FP32_REL * mag if prec == PREC_BF16 else PARITY_REL * mag + 1e-30
    return A, W, b, ref, tol


def hm_check(out, ref, tol, B, L, H, prec, what):
    """the whole head-major buffer of run_gemm: every (image, q | k | v head) unit is Lp = round_up(L, 8) rows of 64; rows [L, Lp) and the space
    behind the image keep their canary bytes"""
    Lp = round_up(L, 8)
    n = B * 3 * H * Lp * 64
    img = out[:n].reshape(B, 3 * H, Lp, 64)
    vals = np.ascontiguousarray(img[:, :, :L, :])
    got = (from_bf16_bits(vals) if prec == PREC_BF16 else vals).transpose(0, 2, 1, 3).reshape(B * L, 3 * H * 64)
    r = gate(got, ref, tol, what)
    assert untouched(img[:, :, L:, :]), f"{what}: rows [L, Lp) of a head-major unit written"
    assert untouched(out[n:]), f"{what}: bytes behind the head-major image written"
    return r


def hm_emulate(ref, B, L, H, prec, Lp=None, tok_l=None):
    """the buffer a correct store leaves: the reference rounded to the output type at ((b 3 H + unit) Lp + l) 64 + j, b = row / tok_l, 0xFF bytes
    elsewhere.  Lp, tok_l: the faults of a unit pitch rounded up to 16 rows and of an image index taken with tok_l = N"""
    Lp8 = round_up(L, 8)
    Lp, tok_l = Lp or Lp8, tok_l or L
    size = (B * 3 * H * Lp8 + 64) * 64
    vals = bf16_bits(ref.astype(np.float32)) if prec == PREC_BF16 else ref.astype(np.float32).view(np.uint32)
    out = np.full(size, NAN16 if prec == PREC_BF16 else NAN32, vals.dtype)
    row, col = np.arange(B * L)[:, None], np.arange(3 * H * 64)[None, :]
    b, l = row // tok_l, row % tok_l
    idx = ((b * 3 * H + col // 64) * Lp + l) * 64 + col % 64
    ok = idx < size
    out[idx[ok]] = vals[ok]
    return out if prec == PREC_BF16 else out.view(np.float32)


@gpu
@pytest.mark.parametrize("D,L,B", HM_CASES)
def test_head_major_qkv_store_at_long_lengths(D, L, B):
    """bf16 with tile128 forced to 1 and, where the 256 x 256 kernel takes the shape, to 0 (launch_gemm gives a head-major store to gemm256
    wherever the shape fits it, whatever tile128 says, and to the 128 x 128 kernel elsewhere); the fp32 parity kernel"""
    H, M, N = D // 64, B * L, 3 * D
    bias = (D, L, B) == HM_BIAS
    epi = EPI_BIAS_STORE if bias else EPI_STORE
    A, W, b, ref, tol = hm_case(D, L, B, bias, PREC_BF16)
    q, e = C.c_int(), C.c_int()
    fits256 = ks.ctx().lib.dd_plan_rows(M, N, D, 256, C.byref(q), C.byref(e)) == _lib.DD_OK
    ratios = {}
    for t in (1, 0) if fits256 else (1,):
        _, out, _, _, _ = run_gemm(A, W, b, None, epi, tile128=t, hm=(L, H))
        ratios[f"bf16 tile128={t}"] = hm_check(out, ref, tol, B, L, H, PREC_BF16, f"head-major D={D} L={L} B={B} tile128={t}")
    if (D, L, B) in HM_FP32:
        A, W, b, ref, tol = hm_case(D, L, B, bias, PREC_FP32)
        _, out, _, _, _ = run_gemm(A, W, b, None, epi, prec=PREC_FP32, hm=(L, H))
        ratios["fp32"] = hm_check(out, ref, tol, B, L, H, PREC_FP32, f"head-major fp32 D={D} L={L} B={B}")
    print(f"head-major D={D} L={L} B={B} bias={bias} gemm256 fits={fits256}: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    report("head-major qkv store", f"D={D} L={L} B={B}", ratios)


# ---------------------------------------------------------------------------------------------------------------- fused block tail
TAIL_GEOMETRIES = [(3, 324, 1, 128), (2, 576, 2, 512), (1, 1024, 1, 128)]      # (B, N, E, D)
TAIL_MODES = ["proj+qkv", "proj+skip+qkv", "last"]                              # block 0, the mid block, the last block of a depth-3 long model
TAIL_POISON = ((3, 324, 1, 128), "proj+skip+qkv")


@gpu
@pytest.mark.parametrize("mode", TAIL_MODES)
@pytest.mark.parametrize("B,N,E,D", TAIL_GEOMETRIES)
def test_block_tail_at_long_geometries(B, N, E, D, mode):
    o = ops_for(B, N, E, D)
    report("fused block tail", f"B={B} N={N} E={E} D={D} {mode}", flat(tail_check(o, tail_run(o, mode))))


@gpu
def test_block_tail_poison_does_not_reach_an_output_at_a_long_geometry():
    """the form of test_block_tail.test_poison_does_not_reach_an_output: a second launch whose slab buffer and padding rows hold 0x7F bytes"""
    (B, N, E, D), mode = TAIL_POISON
    o = ops_for(B, N, E, D)
    a, b = tail_run(o, mode), tail_run(o, mode, poison=0x7F)
    M = o.M
    used = a["plan"][1] * a["plan"][2] * a["plan"][3]
    assert same_bytes(a["xres"][:M], b["xres"][:M]) and same_bytes(a["slab"][:used], b["slab"][:used])
    for k in ("out", "ln", "frag", "tap", "qkv"):
        if a[k] is not None:
            assert same_bytes(a[k], b[k]), (mode, k)
    tail_check(o, b)


# ---------------------------------------------------------------------------------------------------------------- row-resident Linears
# (B, patches, extras, K, k_split, set_x, x offset): mlp.fc2, attn.proj and skip_linear of an embed_dim 768 model of 576 patches, mlp.fc2 at 1024
ROWLIN_LONG = [(2, 576, 1, 3072, 0, 0, 100.0), (2, 576, 1, 768, 0, 0, 0.0), (2, 576, 1, 1536, 768, 1, 0.0), (1, 1024, 2, 3072, 0, 0, 0.0)]


@gpu
@pytest.mark.parametrize("B,N,E,K,k_split,set_x,x_offset", ROWLIN_LONG)
def test_rowlin_at_long_geometries(B, N, E, K, k_split, set_x, x_offset):
    """frag False (a long model never takes the fragment order), the bf16 copy and the LayerNorm on"""
    check_rowlin("rowlin long", B, N, E, K, k_split, set_x, False, True, True, x_offset, seed=B * K + E + N)
    print(f"long geometry | row-resident Linear | B={B} N={N} E={E} K={K} k_split={k_split}: inside check_rowlin's gates (ratios on the line above)")


# ---------------------------------------------------------------------------------------------------------------- split-K, embed_dim 1024
# What Backbone::skip_linear / proj / mlp hand splitk_then_reduce_ln (forward.hip): splits = 2, the slabs added by reduce_ln with tok = (L, extras),
# row-major LayerNorm (fused_qa is off above 288 tokens); (K, K1, resid) = skip_linear (2 D, D, 0), attn.proj (D, D, 1), mlp.fc2 (4 D, 4 D, 1).
# choose_paths asks gemm_splitk_supported for every batch up to max_batch: the row partition of gemm256 needs M = 256 q + e q with e <= 8.
# L = 577 has none (577 = 2 x 256 + 65, 1154 = 4 x 256 + 130), so the embed_dim 1024 model of 576 patches runs the GEMM sequence; L = 1025
# has one for every batch up to 7 (1025 B = 256 x 4 B + B), and that model runs split-K.
SPLITK_D, SPLITK_SPLITS = 1024, 2
SPLITK_LINEARS = {"skip_linear": (2048, 1024, 0), "attn.proj": (1024, 0, 1), "mlp.fc2": (4096, 0, 1)}      # K, K1, resid
GEMM_LINEARS = {"skip_linear": (1024, 2048, 1024, EPI_BIAS_SET), "attn.proj": (1024, 1024, 0, EPI_BIAS_RESID),
                "mlp.fc1": (4096, 1024, 0, EPI_BIAS_GELU), "mlp.fc2": (1024, 4096, 0, EPI_BIAS_RESID)}          # N, K, K1, epilogue


def splitk_supported(M, N, K, K1, splits):
    """gemm.hip gemm_splitk_supported on the host: splits >= 2, whole k tiles per split, and a row partition of the 256 x 256 kernel"""
    q, e = C.c_int(), C.c_int()
    fits = _lib.load().dd_plan_rows(M, N, K, 256, C.byref(q), C.byref(e)) == _lib.DD_OK
    return splits >= 2 and (K // 64) % splits == 0 and (K1 or K) % 64 == 0 and fits


def test_which_embed_dim_1024_models_take_split_k():
    """on the host: no batch of 577-token images has a row partition, every batch of 1 .. 7 images of 1025 tokens has one"""
    for name, (K, K1, _) in SPLITK_LINEARS.items():
        assert not splitk_supported(577, SPLITK_D, K, K1, SPLITK_SPLITS) and not splitk_supported(1154, SPLITK_D, K, K1, SPLITK_SPLITS), name
        assert all(splitk_supported(b * 1025, SPLITK_D, K, K1, SPLITK_SPLITS) for b in range(1, 8)), name


@gpu
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("name", list(SPLITK_LINEARS))
def test_split_k_at_1025_tokens(name, B):
    """M = 1025 and 2050: one tail row per 256-row tile, images that no tile boundary respects"""
    K, K1, resid = SPLITK_LINEARS[name]
    L = 1025
    assert splitk_supported(B * L, SPLITK_D, K, K1, SPLITK_SPLITS)
    ratios = check_split_k(SPLITK_D, K, K1, SPLITK_SPLITS, resid, True, False, L, B, 100.0 if name == "attn.proj" else 0.0, n_patches=L - 1)
    report("split-K + reduce_ln", f"{name} D={SPLITK_D} K={K} K1={K1 or K} splits={SPLITK_SPLITS} L={L} B={B}", ratios)


@gpu
@pytest.mark.parametrize("M", [577, 1154])
@pytest.mark.parametrize("name", list(GEMM_LINEARS))
def test_gemm_sequence_of_the_577_token_embed_dim_1024_model(name, M):
    """the launches that model makes instead (gemm_prefers_128 is false without a row partition, so tile128 = 0, and launch_gemm falls to the
    128 x 128 kernel): ragged last row tiles at M = 577 = 4 x 128 + 65 and 1154 = 9 x 128 + 2"""
    N, K, K1, epi = GEMM_LINEARS[name]
    assert not splitk_supported(M, SPLITK_D, 1024, 0, SPLITK_SPLITS)
    check_linear(f"long geometry | GEMM sequence, embed_dim 1024 | {name}", M, N, K, epi, K1=K1, tile128=0, seed=M + N + K)


# ---------------------------------------------------------------------------------------------------------------- head_dec, patch-rows form
HEAD_CASES = [(512, 48, 2, 578, 2), (768, 48, 2, 577, 1), (1024, 16, 2, 577, 1), (256, 48, 1, 1025, 1)]      # (D, pd, B, L, extras)


def head_rows(M, D, seed):
    """the rows of test_head_dec's patch-rows test: offsets of 0, 50 and 2 000 times their spread, rows 1e-3 wide"""
    x = np.random.default_rng(seed).standard_normal((M, D)).astype(np.float32)
    x[1::4] += 50.0
    x[2::4] += 2000.0
    x[3::4] *= 1e-3
    return x


def head_check(dec, want, L, extras, what):
    """the gate of test_head_dec's patch-rows test: the extra tokens' rows come back NaN (not decoded), the patch rows within HEAD_DEC_REL of
    the largest |dec|"""
    M = dec.shape[0]
    patch = (np.arange(M) % L) >= extras
    assert np.isnan(dec[~patch]).all(), f"{what}: the extra tokens' rows are not left alone"
    err = np.abs(dec[patch] - want[patch])
    scale = np.abs(want[patch]).max()
    assert err.max() <= HEAD_DEC_REL * scale, f"{what}: max err {err.max():.3e} of |dec| max {scale:.2f}"
    return float(err.max() / (HEAD_DEC_REL * scale))


@gpu
@pytest.mark.parametrize("D,pd,B,L,extras", HEAD_CASES)
def test_head_dec_patch_rows_at_long_lengths(D, pd, B, L, extras):
    assert (L - extras) % 16 == 0
    M = B * L
    dec, _, want, _, _ = head_run(M, D, pd, L, extras, head_rows(M, D, M + D), False)
    report("head_dec, patch rows", f"D={D} pd={pd} B={B} L={L} extras={extras}", head_check(dec, want, L, extras, f"head_dec D={D} L={L}"))


# ---------------------------------------------------------------------------------------------------------------- token assembly, generic kernel
EMBED_CASES = [(72, 4, 3, 128, 1, 3), (96, 4, 3, 512, 2, 2), (96, 4, 3, 768, 1, 1), (48, 2, 4, 1024, 1, 2), (128, 4, 3, 128, 1, 1),
               (128, 2, 3, 64, 1, 1)]                                                  # (S, P, C, D, extras, B)
EMBED_T = [999.0, 0.0, 37.0]


@functools.lru_cache(maxsize=2)
def embed_long_case(S, Pz, Cn, D, extras, B):
    """(operands, t, normalize, want, tol) of a case: per-image timesteps, normalized for the class-conditional case"""
    ops = embed_operands(B, Cn, S, Pz, D, extras, 7 * S + D + B)
    t = np.asarray(EMBED_T[:B], np.float64)
    normalize = int(extras == 2)
    want, tol = embed_ref(*ops, t, extras, normalize)
    return ops, t, normalize, want, tol


def embed_gate(got, want, tol, extras, what):
    """the two gates of test_row_kernels.embed_case on [B, L, D] rows: the time token's columns, the patch and label tokens'"""
    is_time = np.arange(want.shape[1]) == extras - 1
    return {"time token": gate(got[:, is_time], want[:, is_time], tol[:, is_time], what + " time token"),
            "patch and label tokens": gate(got[:, ~is_time], want[:, ~is_time], tol[:, ~is_time], what + " patch and label tokens")}


def embed_emulate(ops, want, S, Pz, extras, fault=None):
    """what a correct kernel returns (the reference in fp32), or the tokens of a kernel that takes the patch grid 16 wide ("w16": patch n read
    at row n / 16, column n % 16) or with gy and gx exchanged ("swap")"""
    pos = ops[3].astype(np.float64)
    got = want.copy()
    if fault:
        g = S // Pz
        n = np.arange(g * g)
        gy, gx = ((n // 16) % g, n % 16) if fault == "w16" else (n % g, n // g)
        tokens = want[:, extras:] - pos[extras:]
        got[:, extras:] = tokens[:, gy * g + gx] + pos[extras:]
    return got.astype(np.float32)


@gpu
@pytest.mark.parametrize("S,Pz,Cn,D,extras,B", EMBED_CASES)
def test_embed_generic_at_long_grids(S, Pz, Cn, D, extras, B):
    (x, w, bias, pos, label, y), t, normalize, want, tol = embed_long_case(S, Pz, Cn, D, extras, B)
    xt, _ = run_embed(x, w, bias, pos, label, y, extras, normalize, 1, t_vec=t)
    L = want.shape[1]
    Mp = xt.shape[0] - 8
    what = f"embed S={S} P={Pz} C={Cn} D={D} extras={extras} B={B} (grid {S // Pz} wide, L={L})"
    assert np.all(xt[Mp:] == NAN32), what + ": the rows behind the workspace were written"
    assert not xt[B * L:Mp].any(), what + ": padding rows are not zero"
    report("token assembly, generic kernel", what, embed_gate(xt[:B * L].view(np.float32).reshape(B, L, D), want, tol, extras, what))


# ---------------------------------------------------------------------------------------------------------------- time_embed MLP
TIME_MLP_D = 128
TIME_MLP_CASES = [(325, 1), (4098, 2)]      # (L, extras)


def time_mlp_long_case(L, extras):
    ops = time_mlp_operands(TIME_MLP_D, L, seed=TIME_MLP_D + L + extras)
    t = np.asarray([999.0, 1.0], np.float32)
    return ops, t, time_mlp_tolerance(t, TIME_MLP_D, 1, *ops[:4], ops[4][extras - 1])


@gpu
@pytest.mark.parametrize("L,extras", TIME_MLP_CASES)
def test_time_mlp_at_long_lengths(L, extras):
    """row extras - 1 of every image of L rows is rewritten; every other row keeps its bits"""
    ctx = ks.ctx()
    D, B = TIME_MLP_D, 2
    (w1, b1, w2, b2, pos), t, (want, tol, e32) = time_mlp_long_case(L, extras)
    x0 = np.random.default_rng(L).standard_normal((B, L, D)).astype(np.float32)
    xt = x0.copy()
    ctx.check(ctx.lib.dd_dev_time_mlp(ctx.handle, B, D, L, extras, 1, P(w1), P(b1), P(w2), P(b2), P(pos), P(t), 0.0, P(xt), 0, None, C.byref(C.c_float(0))))
    what = f"time_mlp D={D} B={B} L={L} extras={extras}"
    ratio = gate(xt[:, extras - 1], want, tol, what)
    others = np.arange(L) != extras - 1
    assert np.array_equal(xt[:, others].view(np.uint32), x0[:, others].view(np.uint32)), what + ": another row changed"
    report("time_mlp", what + f" (e32 {e32:.2e})", ratio)


# ---------------------------------------------------------------------------------------------------------------- the step tail
FINAL_CASES = [(3, 4, 72, 1), (3, 4, 72, 2), (3, 4, 96, 1), (3, 4, 128, 1), (4, 2, 128, 1)]      # (C, P, S, B)
FINAL_FULLEST = [(3, 4, 72, 1), (3, 4, 128, 1)]


@gpu
@pytest.mark.parametrize("C_,P_,S,B", FINAL_CASES)
def test_step_tail_at_long_sizes(C_, P_, S, B):
    """the forward-only launch (eps_out alone) and, at S = 72 and 128, the fullest step: classifier-free guidance, history, the known region"""
    a = ks.final_head_inputs(C_, P_, S, B=B)
    o = launch(a)
    ratios = {"forward": check_eps(a, o, f"C{C_} P{P_} S{S} B{B} forward")}
    assert untouched(o.x), "the x_out of a forward-only launch"
    assert (o.q.t_out, o.q.t_final_out) == (0, 0)
    if (C_, P_, S, B) in FINAL_FULLEST:
        a = ks.final_head_inputs(C_, P_, S, "cfg", B=B)
        ratios["fullest"], _ = run_step(a, f"C{C_} P{P_} S{S} B{B} cfg fullest", **combo("cfg", True, True))
    report("step tail", f"C={C_} P={P_} S={S} B={B} (L={a['L']})", ratios)


@gpu
def test_philox_ddpm_step_at_128_pixels():
    """the DDPM rule's z at S = 128 for a launch that starts at image 5: pixel ids 5 x 16 384 .. 6 x 16 384 - 1, the counter word = t"""
    case = dict(S=128, B=1, C=3, b0=5, seed=(7 << 32) | 0x9ABCDEF1, ctr=941, z2=False)
    want, _ = ks.final_philox_ref(case["seed"], 1, 3, 128, 5, 941)
    report("step tail", "Philox DDPM step S=128 b0=5", gate(draw(case, ddpm=True), want, PHILOX_BOUND, "the DDPM rule's z at S = 128, b0 = 5"))


# ---------------------------------------------------------------------------------------------------------------- the gates see geometry faults (CPU)
def rejects(fn, *args):
    with pytest.raises(AssertionError):
        fn(*args)


def test_head_major_gate_rejects_geometry_faults():
    """L = 325 (Lp = 328), B = 3, both precisions: the correct store passes; a unit pitch of round_up(L, 16) = 336 rows and an image index
    taken with tok_l = N = 324 are rejected"""
    D, L, B = 128, 325, 3
    H = D // 64
    for prec in (PREC_BF16, PREC_FP32):
        _, _, _, ref, tol = hm_case(D, L, B, False, prec)
        assert hm_check(hm_emulate(ref, B, L, H, prec), ref, tol, B, L, H, prec, "the reference, rounded") <= 1.0
        rejects(hm_check, hm_emulate(ref, B, L, H, prec, Lp=round_up(L, 16)), ref, tol, B, L, H, prec, "Lp rounded up to 16")
        rejects(hm_check, hm_emulate(ref, B, L, H, prec, tok_l=L - 1), ref, tol, B, L, H, prec, "image index with tok_l = N")


def test_block_tail_gates_reject_geometry_faults():
    """(B, N, E, D) = (3, 324, 1, 128): the emulated kernel passes every gate in the three modes a long model launches; the image index taken
    with tok_l = N and the last ragged 32-row group (4 rows) of every image left out are rejected in each"""
    o = ops_for(3, 324, 1, 128)
    for mode in TAIL_MODES:
        worst = max(flat(tail_check(o, tail_emulate(o, mode))).values())
        assert worst < 1.0, (mode, worst)
        for bug in ("tok_l", "ragged"):
            rejects(tail_check, o, tail_emulate(o, mode, bug=bug))


def rows_of_the_image_above(v, B, L, E):
    """the fault of an image index taken with tok_l = N: image b's patch rows hold what belongs b E rows further up"""
    M = B * L
    r = np.arange(M)
    patch = r % L >= E
    bad = v.copy()
    bad[patch] = v[r[patch] - E * (r[patch] // L)]
    return bad


def test_row_linear_gates_reject_geometry_faults():
    """the x gate of check_rowlin and of check_split_k, FP32_REL (|A| . |W|^T + |bias| + |x|), on B = 2 images of 577 tokens: the reference in
    fp32 passes; image 1's patch rows taken one row up (tok_l = N), and the one tail row of a 256-row tile left out of the second slab
    (M = 1025), are rejected"""
    B, N, E, K = 2, 576, 1, 768
    L, M = N + E, B * (N + E)
    A, W, bias, x_in = operands(M, 768, K, 5)
    acc, absum = linear_ref(A, W)
    xref = acc + bias + x_in.astype(np.float64)
    tx = FP32_REL * (absum + np.abs(bias) + np.abs(x_in))
    assert gate(xref.astype(np.float32), xref, tx, "fp32 of the reference") < 1.0
    rejects(gate, rows_of_the_image_above(xref, B, L, E).astype(np.float32), xref, tx, "rowlin: image index with tok_l = N")
    M, D, K = 1025, 256, 512
    A, W, bias, x_in = operands(M, D, K, 6)
    acc, absum = linear_ref(A, W)
    xref = acc + bias + x_in.astype(np.float64)
    tx = FP32_REL * (absum + np.abs(bias) + np.abs(x_in))
    s1, a1 = linear_ref(A, W, k0=K // 2, k1=K)
    assert gate(xref.astype(np.float32), xref, tx, "fp32 of the reference") < 1.0
    bad = xref.copy()
    bad[M - 1] -= s1[M - 1]
    rejects(gate, bad.astype(np.float32), xref, tx, "split-K: the tail row without its second slab")
    slab1 = s1.copy()
    slab1[M - 1] = 0.0
    rejects(gate, slab1.astype(np.float32), s1, FP32_REL * a1, "split-K: slab 1 of the tail row not written")


def test_head_dec_gate_rejects_extra_rows_decoded_as_patch_rows():
    """(D, pd, B, L, E) = (512, 48, 2, 578, 2): the reference in fp32 with NaN in the extra-token rows passes; a kernel that places image 1's
    units at row L + 0 instead of L + tok_e decodes its two extra-token rows and leaves its last two patch rows alone: rejected"""
    D, pd, B, L, E = 512, 48, 2, 578, 2
    M = B * L
    r = np.random.default_rng(8)
    x = head_rows(M, D, 9)
    g, b = (1.0 + 0.2 * r.standard_normal(D)).astype(np.float32), (0.1 * r.standard_normal(D)).astype(np.float32)
    w, bias = (r.standard_normal((pd, D)) / np.sqrt(D)).astype(np.float32), (0.1 * r.standard_normal(pd)).astype(np.float32)
    want = head_reference(x, g, b, w, bias)
    patch = (np.arange(M) % L) >= E
    good = want.astype(np.float32)
    good[~patch] = np.nan
    assert head_check(good, want, L, E, "the reference in fp32") < 1.0
    bad = good.copy()
    bad[L:L + E] = want[L:L + E]
    bad[2 * L - E:] = np.nan
    rejects(head_check, bad, want, L, E, "image 1 decoded from its first row")
    bad = good.copy()
    bad[L:L + E] = want[L:L + E]
    rejects(head_check, bad, want, L, E, "image 1's extra-token rows decoded too")


def test_embed_gates_reject_geometry_faults():
    """S = 72, P = 4 (a grid 18 wide, 324 patches), B = 3, and the class-conditional S = 96 case: the reference in fp32 passes; the grid taken
    16 wide, gy and gx exchanged, and pos_embed shifted by one row (embed_ref's pos_shift: the extra tokens' rows) are rejected"""
    for S, Pz, Cn, D, extras, B in (EMBED_CASES[0], EMBED_CASES[1]):
        ops, t, normalize, want, tol = embed_long_case(S, Pz, Cn, D, extras, B)
        worst = max(embed_gate(embed_emulate(ops, want, S, Pz, extras), want, tol, extras, "the reference in fp32").values())
        assert worst < 1.0, worst
        for fault in ("w16", "swap"):
            rejects(embed_gate, embed_emulate(ops, want, S, Pz, extras, fault), want, tol, extras, fault)
        shifted, _ = embed_ref(*ops, t, extras, normalize, pos_shift=1)
        rejects(embed_gate, shifted.astype(np.float32), want, tol, extras, "pos shifted by one row")


def test_time_mlp_gate_rejects_the_neighbouring_pos_row():
    """L = 4098, extras = 2: a float32 evaluation passes; the time token with the pos_embed row of token `extras` is rejected"""
    L, extras = TIME_MLP_CASES[1]
    (w1, b1, w2, b2, pos), t, (want, tol, _) = time_mlp_long_case(L, extras)
    assert gate(time_mlp_ref(t, TIME_MLP_D, 1, w1, b1, w2, b2, pos[extras - 1], np.float32), want, tol, "float32 evaluation") < 1.0
    rejects(gate, time_mlp_ref(t, TIME_MLP_D, 1, w1, b1, w2, b2, pos[extras]), want, tol, "the pos row of the first patch token")


def final_emulate(a, want, drop_ragged=False):
    """the buffers of launch() as a correct forward-only launch leaves them: eps = the reference in fp32, 0xFF bytes behind image B.
    drop_ragged: a tile grid of S / 16 rounded DOWN per side, the pixels of the ragged last tile row and column never written"""
    B, Cn, S = a["B"], a["C"], a["S"]
    e = want.astype(F32)
    if drop_ragged:
        e[..., S // 16 * 16:, :] = ff(1)[0]
        e[..., :, S // 16 * 16:] = ff(1)[0]
    o = Out()
    o.img = Cn * S * S
    o.eps = np.concatenate([e.reshape(-1), ff(o.img + 8)])
    return o


def test_step_tail_gate_rejects_a_dropped_ragged_tile():
    """S = 72 = 4.5 tiles of 16 pixels: check_eps accepts the reference in fp32 and rejects 4 x 4 tiles"""
    a = ks.final_head_inputs(3, 4, 72, B=1)
    want, _ = ks.final_eps64(**a)
    assert check_eps(a, final_emulate(a, want), "the reference in fp32") < 1.0
    rejects(check_eps, a, final_emulate(a, want, drop_ragged=True), "floor(S / 16) tiles per side")
