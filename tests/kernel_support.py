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
