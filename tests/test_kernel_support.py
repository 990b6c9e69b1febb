"""CPU tests of tests/kernel_support.py, the one copy of what every per-element kernel test rests on: the host's bf16 rounding against torch's,
the bf16 ulp, the gate's predicate at and around its bound, and the two fragment orders against a literal element-by-element evaluation of the
formulas in include/duodiff_dev.h (dd_dev_block_tail_frag)."""
import numpy as np
import pytest
import torch

from kernel_support import bf16, bf16_bits, from_bf16_bits, frag16_index, frag32_index, gate, to_frag, ulp_bf16, unfrag


def _sample():
    """4096 normals over 2^+-20; every exact tie (low half 0x8000) above a normal upper half, of both parities and both signs, and the values
    one fp32 ulp either side of each; +-0, the largest finite bf16, the smallest normal"""
    r = np.random.default_rng(0)
    normals = (r.standard_normal(4096) * 2.0 ** r.integers(-20, 21, 4096)).astype(np.float32)
    hi = np.arange(0x0080, 0x7F80, dtype=np.uint32)
    ties = (np.concatenate([hi, hi | 0x8000]) << 16) | 0x8000
    edge = np.array([0x00000000, 0x80000000, 0x7F7F0000, 0xFF7F0000, 0x00800000, 0x80800000], np.uint32)
    return np.concatenate([normals, np.concatenate([ties, ties - 1, ties + 1, edge]).view(np.float32)])


def test_bf16_equals_torch_bit_for_bit():
    x = _sample()
    want = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
    assert np.array_equal(bf16(x).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(bf16_bits(x), want.view(np.uint32) >> 16)
    assert np.array_equal(from_bf16_bits(bf16_bits(x)).view(np.uint32), want.view(np.uint32))


def test_ulp_bf16_is_the_distance_to_the_next_bf16():
    x = _sample()
    b = np.abs(bf16(x))
    b = b[b < from_bf16_bits(np.uint16(0x7F7F))]             # (the largest finite bf16 has no finite neighbour above it)
    above = from_bf16_bits(bf16_bits(b) + np.uint16(1))
    want = np.where(b == 0, 0.0, above.astype(np.float64) - b.astype(np.float64))
    assert np.array_equal(ulp_bf16(b), want)
    assert np.array_equal(ulp_bf16(x), ulp_bf16(bf16(x)))   # taken at bf16(y), whatever y
    assert ulp_bf16(np.float32(0.0)) == 0.0 and ulp_bf16(np.float32(-0.0)) == 0.0


def test_gate_predicate_and_message():
    tol = np.full((4, 6), 0.25)
    zero = np.zeros((4, 6))
    assert gate(tol, zero, tol, "err == tol exactly") == 1.0
    over = tol.copy()
    over[2, 3] = np.nextafter(0.25, 1.0)
    with pytest.raises(AssertionError, match=r"1 of 24 elements out of bound; first at \(2, 3\)") as e:
        gate(over, zero, tol, "one ulp above")
    assert "one ulp above" in str(e.value) and "bound 0.25" in str(e.value) and "largest error / bound 1.000" in str(e.value)
    nan = zero.copy()
    nan[1, 0] = np.nan
    with pytest.raises(AssertionError, match=r"first at \(1, 0\)"):
        gate(nan, zero, np.inf, "NaN under an infinite bound")
    assert gate(zero + 0.5, zero, np.inf, "an infinite bound") == 0.0
    # broadcasting: a scalar, a per-column bound
    assert gate(zero + 0.125, zero, 0.25, "scalar bound") == 0.5
    col = np.array([1.0, 2.0, 4.0, 8.0, 16.0, 32.0])
    assert gate(zero + 1.0, zero, col, "per-column bound") == 1.0
    bad = zero + 1.0
    bad[3, 1] = 2.5
    with pytest.raises(AssertionError, match=r"first at \(3, 1\).*bound 2\.0"):
        gate(bad, zero, col, "per-column bound")
    assert gate(zero + 1.0, zero, 0.0 * col + 2.0, "ratio") == 0.5
    # nothing to compare
    assert gate(np.zeros((0, 6)), np.zeros((0, 6)), np.zeros((0, 6)), "empty") == 0.0
    assert gate(np.zeros((0, 6)), np.zeros((0, 6)), 1.0, "empty, scalar bound") == 0.0


@pytest.mark.parametrize("D", [64, 512])
def test_fragment_orders_are_the_header_formulas(D):
    rows = 64                                                # two 32-row groups: the group stride is exercised
    i16, i32 = frag16_index(rows, D), frag32_index(rows, D)
    assert i16.shape == i32.shape == (rows, D)
    seen16, seen32 = np.zeros(rows * D, bool), np.zeros(rows * D, bool)
    for group in range(rows // 32):
        for lane in range(64):
            p = 32 * group + (lane & 31)
            for ks in range(D // 16):                        # bf16: element ((group (D / 16) + ks) 64 + lane) 8 + j = column 16 ks + 8 (lane >> 5) + j
                for j in range(8):
                    el = ((group * (D // 16) + ks) * 64 + lane) * 8 + j
                    assert i16[p, 16 * ks + 8 * (lane >> 5) + j] == el
                    seen16[el] = True
            for t in range(D // 32):                         # fp32: element (((group (D / 32) + t) 4 + g) 64 + lane) 4 + e = column 32 t + 8 g + 4 (lane >> 5) + e
                for g in range(4):
                    for e in range(4):
                        el = (((group * (D // 32) + t) * 4 + g) * 64 + lane) * 4 + e
                        assert i32[p, 32 * t + 8 * g + 4 * (lane >> 5) + e] == el
                        seen32[el] = True
    assert seen16.all() and seen32.all()
    x = np.random.default_rng(D).integers(0, 0x10000, (rows, D)).astype(np.uint16)
    for index in (frag16_index, frag32_index):
        fr = to_frag(x, D, index=index)
        assert fr.shape == (rows * D,) and np.array_equal(unfrag(fr, rows // 32, D, index=index), x)
        assert np.array_equal(to_frag(unfrag(fr, rows // 32, D, index=index), D, index=index), fr)
        assert np.array_equal(unfrag(np.concatenate([fr, fr[:D]]), rows // 32, D, index=index), x)      # a buffer longer than its groups
    good, swapped = to_frag(x, D).reshape(-1, 8), to_frag(x, D, swap_halves=True).reshape(-1, 8)
    assert (good != swapped).any(1).all(), "a 16-byte piece survives the exchange of the lane halves"
    assert np.array_equal(swapped.reshape(-1, 2, 32, 8)[:, ::-1].reshape(-1, 8), good)
