"""The KL-VAE's GEMM launches (csrc/vae.hip: Net::gemm / conv3 / attn, the weight repack of dd_vae_finalize) per element against float64.

Part 1: every (N, K, epilogue) the decoder and the encoder launch, through dd_dev_gemm under check_linear of tests/test_gemm_path.py.
VAE_GEMMS below is written out from vae.hip; test_case_list_is_the_models (CPU) derives the same list from vae_param_shapes() /
vae_encoder_param_shapes().  The attention block's three launches per image run at HW = 64, 576 and 1024 pixels: V^T = Wv . h^T (the weight
is the A operand, EPI_STORE, ldo = HW), S = Q . K^T (EPI_BIAS_SET with a NULL bias, into a buffer that holds canary bytes) and
O = P . V^T^T + b_v (P: rows of a real softmax, V^T shifted to mean 2).  bf16 shapes the persistent 256 x 256 kernel takes run with
tile128 = 1, tile128 = 0 and, at M = 2048 on a grid of 8 workgroups, tile128 = -1; the two kernels must agree bit for bit (see part 3).
Part 2: every GEMM launch of a real decode (8 x 8 latents) and encode (64 x 64 pixels) of B = 2 images, copied out by dd_dev_vae_trace and
gated in place: float64 of the launch's OWN operands, and every weight operand bit for bit against a numpy restatement of the repack.
Part 3: a bf16 image does not depend on the chunk it was decoded / encoded in (max_chunk = 4, five images: chunks of 4 and 1).

Gates (imported, none measured on the kernel): fp32 results of the bf16 kernels FP32_REL = 2^-16 of |A| . |W|^T + |bias| + |x_in|, the fp32
parity kernels PARITY_REL = 2^-20 of the same sum, bf16 outputs one bf16 ulp on top.  test_gates_are_fair (CPU) accumulates every class of
operands in float32 in the kernel's grouping (16 k per add for v_mfma_f32_32x32x16_bf16, 2 k per add for v_mfma_f32_32x32x2_f32; ascending k)
and asserts that this arithmetic alone stays within HALF the gate.  Where it does not, the class takes the a-priori bound
(K / g + 2) 2^-24 of the same sum instead (g = 16 / 2: one rounding per add, + bias, + x), and the test asserts that as well:
  * fp32, O = P . V^T^T + b_v with an all-positive P and a V of mean 2, K = HW = 576:  the emulation reaches 2^-19.7 of the sum
    (half of PARITY_REL is 2^-21; the a-priori bound is 2^-15.8),
  * the same at K = HW = 1024: 2^-19.1 (a-priori bound 2^-15.0).  Every partial sum has the sign and the size of the result, so the
    roundings of the 512 adds do not cancel the way they do for centred operands.
Every other class passes with the imported factor and keeps it: centred operands at K = 4608 reach 2^-22.8 in fp32 and 2^-24.1 in the bf16
grouping; the positive O class reaches 2^-20.7 in the bf16 grouping at K = 1024 (half of FP32_REL: 2^-17) and 2^-21.4 in fp32 at K = 64.
"""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import REPO
from kernel_support import FP32_REL, PARITY_REL, PREC_BF16, PREC_FP32, P, U24, bf16, bf16_bits, from_bf16_bits, gate, round_up, softmax_ref, ulp_bf16
from test_gemm_path import EPI_BIAS_RESID, EPI_BIAS_SET, EPI_BIAS_STORE, EPI_NAME, EPI_STORE, check_linear, linear_ref, operands

from duodiff_amd.autoencoder import (FrozenAutoencoderKL, synthetic_vae_encoder_state_dict, synthetic_vae_state_dict, vae_encoder_param_shapes,
                                     vae_param_shapes)

gpu = pytest.mark.gpu
PRECS = {"bf16": PREC_BF16, "fp32": PREC_FP32}
KT = {"bf16": 64, "fp32": 32}                 # the GEMM k-tile in elements (128 bytes), what dd_vae_finalize pads a conv's K to

# ---------------------------------------------------------------------------------------------------------------- the case list
# (N, K) -> the epilogues vae.hip launches it with.  N: cout, 3 -> 4.  K: k k cin (cin 3 -> 4) rounded up to the k-tile; every K of the model
# is the same in both precisions (36 -> 64 either way, the others are multiples of 64).
S_, R_, O_ = EPI_BIAS_SET, EPI_BIAS_RESID, EPI_BIAS_STORE
VAE_GEMMS = {
    (512, 64): (S_,), (128, 64): (S_,),                                                    # decoder / encoder conv_in (9 x 4 = 36 padded)
    (512, 4608): (S_, R_), (256, 4608): (S_,), (8, 4608): (S_,),                           # 512-channel 3x3 convs; encoder conv_out
    (512, 2304): (S_,), (256, 2304): (S_, R_), (128, 2304): (S_,),
    (256, 1152): (S_,), (128, 1152): (S_, R_), (4, 1152): (S_,),                           # decoder conv_out: 3 channels padded to 4
    (512, 512): (O_, R_),                                                                  # attn q, k (bf16 / fp32 copy, ldo = C); proj_out
    (256, 512): (S_,), (512, 256): (S_,), (128, 256): (S_,), (256, 128): (S_,),            # nin_shortcut
}
ATTN_HW = (64, 576, 1024)
ATTN_C = 512
ATTN_KINDS = ("vt", "s", "o")      # V^T: M = C, N = HW, K = C, EPI_STORE, ldo = HW;  S: M = N = HW, K = C, EPI_BIAS_SET, no bias;  O: M = HW, N = C, K = HW, EPI_BIAS_SET


def conv_epilogue(name):
    """the epilogue vae.hip gives the conv `name` (its module path without .weight); None: no GEMM of its own"""
    if name in ("post_quant_conv", "quant_conv") or name.endswith("attn_1.v"):
        return None                                  # point-wise kernels (launch_vae_input / _moments); v: the per-image attention triple
    if name.endswith(".conv2") or name.endswith("attn_1.proj_out"):
        return EPI_BIAS_RESID
    if name.endswith("attn_1.q") or name.endswith("attn_1.k"):
        return EPI_BIAS_STORE
    return EPI_BIAS_SET                              # conv_in, conv1, nin_shortcut, upsample.conv, downsample.conv, conv_out


def conv_nk(shape, prec):
    co, ci, k, _ = shape
    return (4 if co == 3 else co), round_up(k * k * (4 if ci == 3 else ci), KT[prec])


def all_conv_shapes():
    shp = dict(vae_param_shapes())
    shp.update(vae_encoder_param_shapes())
    return {n[:-len(".weight")]: s for n, s in shp.items() if len(s) == 4}


def test_case_list_is_the_models():
    """every conv weight of both directions maps to exactly one (N, K) of VAE_GEMMS with its epilogue, in both precisions; nothing in the list
    is unused; the attention triple is there; the distinct pairs are the 16 the model has"""
    for prec in PRECS:
        seen = {}
        for name, shape in all_conv_shapes().items():
            epi = conv_epilogue(name)
            if epi is None:
                continue
            nk = conv_nk(shape, prec)
            assert nk in VAE_GEMMS and epi in VAE_GEMMS[nk], (name, nk, epi)
            seen.setdefault(nk, set()).add(epi)
        assert {k: tuple(sorted(v)) for k, v in seen.items()} == {k: tuple(sorted(v)) for k, v in VAE_GEMMS.items()}
    assert len(VAE_GEMMS) == 16 and sum(len(v) for v in VAE_GEMMS.values()) == 20
    v = all_conv_shapes()
    assert v["decoder.mid.attn_1.v"] == v["encoder.mid.attn_1.v"] == (ATTN_C, ATTN_C, 1, 1) and ATTN_KINDS == ("vt", "s", "o")
    # the source the list was written from still says what the list says
    src = (REPO / "duodiff_amd" / "csrc" / "vae.hip").read_text()
    assert "w.cout == 3 ? 4 : w.cout" in src and "cs = ci == 3 ? 4 : ci" in src and "kpad = (K + kt - 1) / kt * kt" in src
    assert len(re.findall(r"launch_gemm<T>\(", src)) == 3      # Net::launch (plain and traced): every GEMM leaves through it


# ---------------------------------------------------------------------------------------------------------------- operands of every class
def conv_ops(M, N, K, seed):
    """a conv launch: im2col rows ~ N(0, 1), weights ~ N(0, 1 / K), bias, residual stream.  K = 64 is conv_in: 36 real columns, the padding
    zero on both sides.  N = 4 is the decoder's conv_out: the fourth weight row and bias are zero, so column 3 must come back as exactly 0."""
    A, W, bias, x = operands(M, N, K, seed)
    if K == 64:
        A[:, 36:] = 0
        W[:, 36:] = 0
    if N == 4:
        W[3] = 0
        bias[3] = 0
    return A, W, bias, x


def attn_ops(kind, HW, seed, C_=ATTN_C):
    """the operands of one launch of the attention triple (module docstring)"""
    r = np.random.default_rng(seed)
    if kind == "vt":
        return (r.standard_normal((C_, C_)) / np.sqrt(C_)).astype(np.float32), r.standard_normal((HW, C_), dtype=np.float32), None, None
    if kind == "s":
        return r.standard_normal((HW, C_), dtype=np.float32), r.standard_normal((HW, C_), dtype=np.float32), None, None
    sigma = np.where(np.arange(HW) % 2 == 0, 0.5, 3.0)[:, None]                          # rows of N(0, 0.5) and of N(0, 3) scores
    p, _ = softmax_ref((sigma * r.standard_normal((HW, HW))).astype(np.float32), 1.0)
    vt = (2.0 + r.standard_normal((C_, HW))).astype(np.float32)
    return p.astype(np.float32), vt, (0.5 * r.standard_normal(C_)).astype(np.float32), None


def attn_shape(kind, HW, C_=ATTN_C):
    """(M, N, K, epilogue, ldo)"""
    return {"vt": (C_, HW, C_, EPI_STORE, HW), "s": (HW, HW, C_, EPI_BIAS_SET, None), "o": (HW, C_, HW, EPI_BIAS_SET, None)}[kind]


# ---------------------------------------------------------------------------------------------------------------- the gates and their fairness
APRIORI = {("o", 576, "fp32"), ("o", 1024, "fp32")}      # (kind, K, precision): classes whose float32 emulation exceeds half the imported factor


def rel_of(kind, K, prec):
    """the factor of |A| . |W|^T + |bias| + |x_in| for a class of launches: imported, or the a-priori bound where APRIORI names the class"""
    if (kind, K, prec) in APRIORI:
        return (K / (16 if prec == "bf16" else 2) + 2) * U24
    return FP32_REL if prec == "bf16" else PARITY_REL


def emulate(A, W, bias, x_in, prec):
    """the launch in float32 in the kernel's grouping: g products summed, one float32 add per group, then + bias, then x + ."""
    q = bf16 if prec == "bf16" else (lambda a: a)
    a, w = q(A).astype(np.float64), q(W).astype(np.float64)
    g = 16 if prec == "bf16" else 2
    acc = np.zeros((A.shape[0], W.shape[0]), np.float32)
    for k0 in range(0, A.shape[1], g):
        acc = (acc.astype(np.float64) + a[:, k0:k0 + g] @ w[:, k0:k0 + g].T).astype(np.float32)
    if bias is not None:
        acc = acc + bias.astype(np.float32)
    if x_in is not None:
        acc = x_in.astype(np.float32) + acc
    assert acc.dtype == np.float32
    return acc


def emulation_ratio(A, W, bias, x_in, prec):
    """max over the elements of |emulation - float64| / (|A| . |W|^T + |bias| + |x_in|)"""
    acc, absum = linear_ref(A, W, PRECS[prec])
    ref = acc + (bias if bias is not None else 0.0) + (x_in if x_in is not None else 0.0)
    mag = absum + (np.abs(bias) if bias is not None else 0.0) + (np.abs(x_in) if x_in is not None else 0.0)
    return float((np.abs(emulate(A, W, bias, x_in, prec) - ref) / mag).max())


def fairness_classes():
    """(kind, K, operands at 96 rows x 64 columns) of every class of part 1: the error of an accumulation depends on K and on the operands'
    signs, not on M or N"""
    for K in sorted({k for _, k in VAE_GEMMS}):
        A, W, bias, x = conv_ops(96, 64, K, 100 + K)
        yield "conv", K, (A, W, bias, x)                       # EPI_BIAS_RESID: the epilogue with the most roundings
    for kind in ("vt", "s"):
        A, W, _, _ = attn_ops(kind, 96, 7)
        yield kind, ATTN_C, (A[:96], W[:64], None, None)
    for HW in ATTN_HW:
        A, W, bias, _ = attn_ops("o", HW, 8)
        yield "o", HW, (A[:96], W[:64], bias[:64], None)


def test_gates_are_fair():
    """float32 arithmetic in the kernel's grouping stays within half of every class's gate; a class has the a-priori bound if and only if it
    does not stay within half the imported factor"""
    for prec in PRECS:
        imported = FP32_REL if prec == "bf16" else PARITY_REL
        for kind, K, ops in fairness_classes():
            e = emulation_ratio(*ops, prec)
            print(f"vae gemm | fairness | {prec} {kind} K={K}: float32 emulation 2^{np.log2(max(e, 1e-300)):.1f} of the sum, gate 2^{np.log2(rel_of(kind, K, prec)):.1f}")
            assert e <= 0.5 * rel_of(kind, K, prec), (prec, kind, K, e)
            assert ((kind, K, prec) in APRIORI) == (e > 0.5 * imported), (prec, kind, K, e)


def test_gates_reject_the_faults_of_these_shapes():
    """the gates of part 1, applied to five perturbed references at the shapes of the VAE, reject each"""
    def gates(ref, absum, bias, x_in, rel):
        tx = rel * (absum + (np.abs(bias) if bias is not None else 0.0) + (np.abs(x_in) if x_in is not None else 0.0))
        return tx, ulp_bf16(ref) + tx

    def rejected(bad, ref, tx, tout, what, fp32_only=False):
        assert gate(ref.astype(np.float32), ref, tx, "the reference in fp32") < 1.0
        with pytest.raises(AssertionError):
            gate(bad.astype(np.float32), ref, tx, what)
        if not fp32_only:
            with pytest.raises(AssertionError):
                gate(bf16(bad.astype(np.float32)), ref, tout, what + " (bf16 copy)")

    for prec in PRECS:
        # 1: the last k-tile of K = 4608 dropped
        M, N, K = 64, 512, 4608
        A, W, bias, x_in = conv_ops(M, N, K, 1)
        acc, absum = linear_ref(A, W, PRECS[prec])
        ref = acc + bias + x_in
        tx, tout = gates(ref, absum, bias, x_in, rel_of("conv", K, prec))
        last, _ = linear_ref(A, W, PRECS[prec], k0=K - KT[prec], k1=K)
        rejected(ref - last, ref, tx, tout, "last k-tile dropped")
        # 2: M = 576, one row of the ragged last 128-row tile holds the clamped row's (M - 1) result
        M, N, K = 576, 128, 1152
        A, W, bias, x_in = conv_ops(M, N, K, 2)
        acc, absum = linear_ref(A, W, PRECS[prec])
        ref = acc + bias
        tx, tout = gates(ref, absum, bias, None, rel_of("conv", K, prec))
        bad = ref.copy()
        bad[570] = ref[575]
        rejected(bad, ref, tx, tout, "row 570 from the clamped row")
        # 3: N = 4, column 3 (zero weight row, zero bias) written with column 0's bias
        M, N, K = 100, 4, 1152
        A, W, bias, _ = conv_ops(M, N, K, 3)
        acc, absum = linear_ref(A, W, PRECS[prec])
        ref = acc + bias
        tx, tout = gates(ref, absum, bias, None, rel_of("conv", K, prec))
        assert np.all(ref[:, 3] == 0) and np.all(tx[:, 3] == 0)
        bad = ref.copy()
        bad[:, 3] += bias[0]
        rejected(bad, ref, tx, tout, "column 3 with column 0's bias", fp32_only=True)
        # 4: O = P . V^T^T without b_v;  5: S with a stale bias slot added where the bias is null
        for HW in ATTN_HW:
            A, W, bias, _ = attn_ops("o", HW, 4)
            acc, absum = linear_ref(A, W, PRECS[prec])
            tx, tout = gates(acc + bias, absum, bias, None, rel_of("o", HW, prec))
            rejected(acc, acc + bias, tx, tout, "O without the bias of v", fp32_only=True)
            A, W, _, _ = attn_ops("s", HW, 5)
            acc, absum = linear_ref(A, W, PRECS[prec])
            tx, tout = gates(acc, absum, None, None, rel_of("s", ATTN_C, prec))
            stale = operands(1, HW, 64, 6)[2]
            rejected(acc + stale, acc, tx, tout, "S with a stale bias slot", fp32_only=True)


# ---------------------------------------------------------------------------------------------------------------- part 1 on the GPU
def m_values(N):
    """576: a 24 x 24 latent, ragged last 128-row tile; 1024: whole tiles; 64: an 8 x 8 latent, less than a tile; the narrow outputs also at
    1100 and 4097 rows"""
    return (576, 1024, 64) + ((1100, 4097) if N <= 128 else ())


def run_ways(name, M, N, K, epi, prec, ops, rel, ldo=None, persistent_at=None):
    """the launch under check_linear: fp32 once; bf16 shapes the 256 x 256 kernel takes with tile128 = 1 and 0 -- bit for bit the same x and
    out -- and (persistent_at: its own operands of that many rows) with tile128 = -1 on a grid of 8 workgroups.  Returns the largest ratio"""
    worst = {}

    def one(tag, M_, ops_, **kw):
        rep = {}
        res = check_linear(f"vae gemm | {name} | {prec} {tag}", M_, N, K, epi, prec=PRECS[prec], ldo=ldo, ops=ops_, rel=rel, report=rep, **kw)
        for k, v in rep.items():
            worst[k] = max(worst.get(k, 0.0), v)
        return res

    if prec == "fp32" or N % 256 or M < 256:
        one("", M, ops)
    else:
        x1, o1 = one("tile128=1", M, ops, tile128=1)
        x0, o0 = one("tile128=0", M, ops, tile128=0)
        assert np.array_equal(x1.view(np.uint32), x0.view(np.uint32)), f"{name}: x differs between the 128 x 128 and the 256 x 256 kernel"
        assert np.array_equal(o1, o0), f"{name}: the bf16 output differs between the 128 x 128 and the 256 x 256 kernel"
    if persistent_at:
        Mp, opsp = persistent_at
        one("tile128=-1 num_cus=8", Mp, opsp, tile128=-1, num_cus=8)
    return worst


CONV_CASES = [(N, K, epi) for (N, K), epis in VAE_GEMMS.items() for epi in epis]


@gpu
@pytest.mark.parametrize("prec", list(PRECS))
@pytest.mark.parametrize("N,K,epi", CONV_CASES)
def test_conv_launches_against_float64_reference(N, K, epi, prec):
    rel = rel_of("conv", K, prec)
    worst = {}
    for M in m_values(N):
        big = None
        if prec == "bf16" and N % 256 == 0 and M == 1024:
            big = (2048, conv_ops(2048, N, K, 31 * N + K + epi))
        w = run_ways(f"conv N={N} K={K} {EPI_NAME[epi]} M={M}", M, N, K, epi, prec, conv_ops(M, N, K, M + N + K + epi), rel,
                     ldo=round_up(N, 8), persistent_at=big)      # (ldo: a multiple of 8 for dd_dev_gemm; only EPI_BIAS_STORE writes out, at ldo = N = C)
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"vae gemm | conv | {prec} N={N} K={K} {EPI_NAME[epi]}: largest error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@gpu
@pytest.mark.parametrize("prec", list(PRECS))
@pytest.mark.parametrize("HW", ATTN_HW)
@pytest.mark.parametrize("kind", ATTN_KINDS)
def test_attention_launches_against_float64_reference(kind, HW, prec):
    M, N, K, epi, ldo = attn_shape(kind, HW)
    ops = attn_ops(kind, HW, 1000 + HW)
    if kind == "o":
        assert ops[0].min() >= 0 and np.allclose(ops[0].sum(-1), 1.0, atol=1e-5) and abs(float(ops[1].mean()) - 2.0) < 0.05
    worst = run_ways(f"attention {kind} HW={HW}", M, N, K, epi, prec, ops, rel_of(kind, K, prec), ldo=ldo,
                     persistent_at=(M, ops) if prec == "bf16" and N % 256 == 0 and M >= 1024 else None)
    print(f"vae gemm | attention | {prec} {kind} HW={HW} (M={M} N={N} K={K} {EPI_NAME[epi]}): largest error / bound "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ---------------------------------------------------------------------------------------------------------------- part 2: the launches of a real pass
def repack(w, prec):
    """dd_vae_finalize's GEMM matrix of a conv weight [cout, cin, k, k]: [cout (3 -> 4), kpad], column t cs + c for tap t = ky k + kx and
    channel c (cs = cin, 3 -> 4), zero padding columns and rows; fp32, or the bits of bf16"""
    w = np.asarray(w, np.float32)
    co, ci, k, _ = w.shape
    cs = 4 if ci == 3 else ci
    N, kpad = conv_nk(w.shape, prec)
    taps = np.zeros((co, k * k, cs), np.float32)
    taps[:, :, :ci] = w.reshape(co, ci, k * k).transpose(0, 2, 1)
    m = np.zeros((N, kpad), np.float32)
    m[:co, :k * k * cs] = taps.reshape(co, k * k * cs)
    return bf16_bits(m) if prec == "bf16" else m


def expected_launches(encode, B, H):
    """the GEMM launches of run_decode (H: the latent size) / run_encode (H: the image size) on B images in issue order, restated from
    vae.hip: dicts of name (the conv's module path, or None), kind, M, N, K, epi, ldo"""
    shapes, out = all_conv_shapes(), []
    state = dict(H=H)

    def conv(name, H_=None):
        co, ci, k, _ = shapes[name]
        M = B * (H_ or state["H"]) ** 2
        epi = conv_epilogue(name)
        out.append(dict(name=name, kind="conv", M=M, N=4 if co == 3 else co, K=k * k * (4 if ci == 3 else ci), epi=epi,
                        ldo=co if epi == EPI_BIAS_STORE else 0, bias=True))

    def res(name):
        if name + ".nin_shortcut" in shapes:
            conv(name + ".nin_shortcut")
        conv(name + ".conv1")
        conv(name + ".conv2")

    def attn(name):
        HW = state["H"] ** 2
        conv(name + ".q")
        conv(name + ".k")
        for _ in range(B):
            for kind in ATTN_KINDS:
                M, N, K, epi, ldo = attn_shape(kind, HW)
                out.append(dict(name=name + ".v" if kind == "vt" else None, kind=kind, M=M, N=N, K=K, epi=epi, ldo=ldo or 0, bias=kind == "o"))
        conv(name + ".proj_out")

    if not encode:
        conv("decoder.conv_in")
        res("decoder.mid.block_1"); attn("decoder.mid.attn_1"); res("decoder.mid.block_2")
        for lv in (3, 2, 1, 0):
            for j in range(3):
                res(f"decoder.up.{lv}.block.{j}")
            if lv != 0:
                state["H"] *= 2
                conv(f"decoder.up.{lv}.upsample.conv")
        conv("decoder.conv_out")
    else:
        conv("encoder.conv_in")
        for lv in range(4):
            for j in range(2):
                res(f"encoder.down.{lv}.block.{j}")
            if lv != 3:
                state["H"] //= 2
                conv(f"encoder.down.{lv}.downsample.conv")
        res("encoder.mid.block_1"); attn("encoder.mid.attn_1"); res("encoder.mid.block_2")
        conv("encoder.conv_out")
    return out


def launch_count(encode, B):
    """from the parameter inventory: every conv weight of the direction but the 1 x 1 point-wise one (post_quant_conv / quant_conv) and
    attn_1.v, whose launch is one of the 3 B of the attention block"""
    shp = vae_encoder_param_shapes() if encode else vae_param_shapes()
    return sum(1 for s in shp.values() if len(s) == 4) - 2 + 3 * B


def test_launch_count_follows_the_parameter_inventory():
    for encode, H in ((0, 8), (1, 64)):
        for B in (1, 2, 4):
            ex = expected_launches(encode, B, H)
            assert len(ex) == launch_count(encode, B)
            named = [e["name"] for e in ex if e["name"]]
            prefix = "encoder." if encode else "decoder."
            assert len(named) == len(set(named)) + B - 1 and set(named) == {n for n in all_conv_shapes() if n.startswith(prefix)}      # (attn_1.v: once per image)
    assert launch_count(0, 2) == 44 and launch_count(1, 2) == 36      # 38 / 30 conv launches + 3 B of the attention block


@pytest.fixture(scope="module")
def full_sd():
    sd = synthetic_vae_state_dict(4321)
    sd.update(synthetic_vae_encoder_state_dict(8765))
    return sd


class Trace:
    """dd_dev_vae_trace on one autoencoder: host buffers sized by a counting pass, one call per ordinal"""

    def __init__(self, ae, encode, x):
        import torch
        from duodiff_amd import _lib as L
        from duodiff_amd.engine import _ptr
        self.ctx, self.h = ae._engine()
        self.encode, self.bf = int(encode), ae.precision == "bf16"
        self.x = x.to(ae.device, torch.float32).contiguous()
        B, hw = self.x.shape[0], self.x.shape[-1]
        self.out = torch.empty((B, 8, hw // 8, hw // 8) if encode else (B, 3, 8 * hw, 8 * hw), device=self.x.device, dtype=torch.float32)
        self.args = (B, hw)
        self._ptr, self.tap = _ptr, L.dd_dev_vae_tap()
        self.tap.ordinal = -1
        self.call()
        t = self.tap
        self.launches = t.launches
        dt = np.uint16 if self.bf else np.float32
        self.A = np.zeros(t.max_a_bytes // dt().itemsize, dt)
        self.W = np.zeros(t.max_w_bytes // dt().itemsize, dt)
        self.o = np.zeros(max(t.max_out_bytes // dt().itemsize, 1), dt)
        self.xb, self.xa = np.zeros(max(t.max_x_bytes // 4, 1), np.float32), np.zeros(max(t.max_x_bytes // 4, 1), np.float32)
        self.bias = np.zeros(4096, np.float32)
        t.A, t.W, t.bias, t.x_before, t.x_after, t.out = P(self.A), P(self.W), P(self.bias), P(self.xb), P(self.xa), P(self.o)
        t.a_bytes, t.w_bytes, t.bias_bytes, t.x_bytes, t.out_bytes = self.A.nbytes, self.W.nbytes, self.bias.nbytes, self.xb.nbytes, self.o.nbytes

    def call(self):
        B, hw = self.args
        self.ctx.check(self.ctx.lib.dd_dev_vae_trace(self.ctx.handle, self.h, self.encode, self._ptr(self.x), self._ptr(self.out), B, hw,
                                                     C.byref(self.tap), None))

    def launch(self, i):
        """dict of launch i: M, N, K, epi, ldo, A / W (fp32 values; A_raw / W_raw: as copied), bias or None, x_before / x_after or out"""
        t = self.tap
        t.ordinal = i
        self.call()
        assert t.tapped == 1 and t.launches == self.launches
        M, N, K = t.M, t.N, t.K
        val = from_bf16_bits if self.bf else (lambda a: a)
        d = dict(M=M, N=N, K=K, epi=t.epilogue, ldo=t.ldo, A_raw=self.A[:M * K].reshape(M, K), W_raw=self.W[:N * K].reshape(N, K),
                 bias=self.bias[:N].copy() if t.has_bias else None)
        d["A"], d["W"] = val(d["A_raw"]), val(d["W_raw"])
        if t.epilogue in (EPI_BIAS_SET, EPI_BIAS_RESID):
            d["x_before"], d["x_after"] = self.xb[:M * N].reshape(M, N), self.xa[:M * N].reshape(M, N)
        else:
            d["out"] = val(self.o[:M * t.ldo].reshape(M, t.ldo))
        return d


@gpu
@pytest.mark.parametrize("prec", list(PRECS))
@pytest.mark.parametrize("encode", [0, 1], ids=["decode", "encode"])
def test_every_gemm_of_a_real_pass_in_place(encode, prec, full_sd):
    """B = 2, 8 x 8 latents / 64 x 64 pixels: every launch's shape and epilogue is the restated one, its result is float64 of ITS operands
    under the gate of its class, its weight operand and bias are the state dict's, repacked, bit for bit; the traced pass returns what the
    plain call returns"""
    import torch
    B, H = 2, 64 if encode else 8
    ae = FrozenAutoencoderKL(full_sd, precision=prec, max_chunk=2, max_latent=8).to("cuda:0")
    g = torch.Generator().manual_seed(5 + encode)
    x = 2.0 * torch.rand(B, 3, H, H, generator=g) - 1.0 if encode else torch.randn(B, 4, H, H, generator=g)
    plain = (ae.encode_moments(x) if encode else ae.decode(x)).cpu().numpy()
    tr = Trace(ae, encode, x)
    assert np.array_equal(tr.out.cpu().numpy().view(np.uint32), plain.view(np.uint32)), "the counting pass differs from the plain call"
    want = expected_launches(encode, B, H)
    assert tr.launches == len(want) == launch_count(encode, B)
    worst, worst_at = 0.0, None
    for i, ex in enumerate(want):
        d = tr.launch(i)
        Kp = round_up(ex["K"], KT[prec])
        assert (d["M"], d["N"], d["K"], d["epi"], d["ldo"], d["bias"] is not None) == (ex["M"], ex["N"], Kp, ex["epi"], ex["ldo"], ex["bias"]), (i, ex)
        what = f"launch {i} ({ex['name'] or ex['kind']})"
        # the weights: the repack of the state dict's tensor, bit for bit
        if ex["kind"] in ("conv", "vt"):
            got_w = d["W_raw"] if ex["kind"] == "conv" else d["A_raw"]
            rp = repack(full_sd[ex["name"] + ".weight"].numpy(), prec)
            assert got_w.shape == rp.shape and np.array_equal(got_w.view(np.uint8), rp.view(np.uint8)), f"{what}: weight operand is not the repack"
        if ex["kind"] == "conv" or ex["kind"] == "o":
            b = full_sd[(ex["name"] if ex["kind"] == "conv" else ("encoder" if encode else "decoder") + ".mid.attn_1.v") + ".bias"].numpy()
            bp = np.zeros(d["N"], np.float32)
            bp[:b.size] = b
            assert np.array_equal(d["bias"].view(np.uint32), bp.view(np.uint32)), f"{what}: bias is not the state dict's"
        assert np.isfinite(d["A"]).all() and np.isfinite(d["W"]).all(), f"{what}: an operand is not finite"
        # the arithmetic: float64 of the launch's own operands (already in the kernel's precision: exact in float64)
        a64, w64 = d["A"].astype(np.float64), d["W"].astype(np.float64)
        ref, mag = a64 @ w64.T, np.abs(a64) @ np.abs(w64).T
        if d["bias"] is not None:
            ref, mag = ref + d["bias"], mag + np.abs(d["bias"])
        if d["epi"] == EPI_BIAS_RESID:
            ref, mag = ref + d["x_before"], mag + np.abs(d["x_before"])
        tol = rel_of(ex["kind"], ex["K"], prec) * mag
        if "out" in d:
            r = gate(d["out"][:, :d["N"]], ref, tol + (ulp_bf16(ref) if prec == "bf16" else 1e-30), what)
        else:
            r = gate(d["x_after"], ref, tol, what)
        if r > worst:
            worst, worst_at = r, what
    after = tr.out.cpu().numpy()
    assert np.array_equal(after.view(np.uint32), plain.view(np.uint32)), "a traced pass differs from the plain call"
    print(f"vae gemm | in place | {'encode' if encode else 'decode'} {prec} B={B}: {tr.launches} launches, largest error / bound {worst:.3f} at {worst_at}")


# ---------------------------------------------------------------------------------------------------------------- part 3: the chunk
@gpu
def test_bf16_image_does_not_depend_on_its_chunk(full_sd):
    """max_chunk = 4, five images in one call (chunks of 4 and 1) against images 0, 3 and 4 alone, bit for bit, decode at 32 x 32 latents and
    encode_moments at 256 x 256 pixels.  launch_gemm chooses between the 128 x 128 and the 256 x 256 kernel from the chunk's M (the N = 256
    convs at 128 x 128 pixels: M = 65536 against 16384); part 1 shows why that cannot show: the two kernels agree bit for bit"""
    import torch
    ae = FrozenAutoencoderKL(full_sd, precision="bf16", max_chunk=4, max_latent=32).to("cuda:0")
    z = torch.randn(5, 4, 32, 32, generator=torch.Generator().manual_seed(31))
    y = ae.decode(z).cpu().numpy()
    assert y.shape == (5, 3, 256, 256) and np.isfinite(y).all()
    for i in (0, 3, 4):
        yi = ae.decode(z[i:i + 1]).cpu().numpy()
        assert np.array_equal(yi[0].view(np.uint32), y[i].view(np.uint32)), f"decode: image {i} differs from its decode alone"
    x = 2.0 * torch.rand(5, 3, 256, 256, generator=torch.Generator().manual_seed(32)) - 1.0
    m = ae.encode_moments(x).cpu().numpy()
    assert m.shape == (5, 8, 32, 32) and np.isfinite(m).all()
    for i in (0, 3, 4):
        mi = ae.encode_moments(x[i:i + 1]).cpu().numpy()
        assert np.array_equal(mi[0].view(np.uint32), m[i].view(np.uint32)), f"encode_moments: image {i} differs from its encode alone"
    print("vae gemm | chunk | bf16 max_chunk=4, 5 images: decode and encode_moments of images 0, 3, 4 equal their single-image calls bit for bit")
