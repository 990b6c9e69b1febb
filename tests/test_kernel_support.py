"""CPU tests of tests/kernel_support.py, the one copy of what every per-element kernel test rests on: the host's bf16 rounding against torch's,
the bf16 ulp, the gate's predicate at and around its bound, and the two fragment orders against a literal element-by-element evaluation of the
formulas in include/duodiff_dev.h (dd_dev_block_tail_frag); and the references of the output head + step launch (tests/test_final_step.py):
the float64 head against torch's conv2d on a rearrange written out index by index, the float32 restatement of step_update.h against a
scalar evaluation with explicit roundings, Philox4x32-10 against the published Random123 vectors, the Box-Muller reference against a scalar
one, and -- on the very inputs the GPU tests use -- that each deliberate error of the reference exceeds the bound the kernel is held to; the
references of the KL-VAE kernels (tests/test_vae_kernels.py) against torch in float64 and their deliberate errors likewise, the emulation of
GroupNorm's one-pass fp32 statistics among them; the references of the early-exit probes (tests/test_ee_probes.py) against torch's float64
modules, their float32 restatements inside the bounds and their deliberate errors outside them."""
import math

import numpy as np
import pytest
import torch

import kernel_support as ks
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


# ---------------------------------------------------------------------------------------------------------------- the output head + step launch
def _rearranged(dec, B, L, extras, C, P, S):
    """ "B (h w) (p1 p2 C) -> B C (h p1) (w p2)" index by index"""
    g = S // P
    d = np.asarray(dec, np.float64).reshape(B, L, P * P * C)
    img = np.zeros((B, C, S, S))
    for h in range(g):
        for w in range(g):
            for p1 in range(P):
                for p2 in range(P):
                    for c in range(C):
                        img[:, c, h * P + p1, w * P + p2] = d[:, extras + h * g + w, (p1 * P + p2) * C + c]
    return torch.from_numpy(img)


def _conv64(img, w, b, C):
    w, b = torch.from_numpy(np.asarray(w, np.float64).reshape(C, C, 3, 3)), torch.from_numpy(np.asarray(b, np.float64))
    return torch.nn.functional.conv2d(img, w, b, padding=1), torch.nn.functional.conv2d(img.abs(), w.abs(), b.abs(), padding=1)


@pytest.mark.parametrize("C,P,S,guided,layers", [(3, 4, 24, None, 1), (4, 2, 8, "cfg", 1), (2, 2, 24, "auto", 1), (1, 8, 16, "auto", 1),
                                                 (3, 2, 16, None, 3), (3, 1, 8, "cfg", 1)])
def test_final_eps64_against_torch_conv2d(C, P, S, guided, layers):
    B = 6 if layers > 1 else 3
    a = ks.final_inputs(C, P, S, B, 2, 11 * S + C, guided, layers=layers)
    got, tol = ks.final_eps64(**a)
    L, e, n = a["L"], a["extras"], 9 * C * C
    if layers > 1:
        lb = a["layer_B"]
        parts = [_conv64(_rearranged(a["dec"][i * lb * L:(i + 1) * lb * L], lb, L, e, C, P, S), a["wconv"][i * a["w_stride"]:][:n],
                         a["bconv"][i * a["b_stride"]:][:C], C) for i in range(layers)]
        c, mc = (torch.cat(v).numpy() for v in zip(*parts))
    else:
        c, mc = (v.numpy() for v in _conv64(_rearranged(a["dec"][:B * L], B, L, e, C, P, S), a["wconv"], a["bconv"], C))
    assert np.isfinite(got).all() and got.shape == (B, C, S, S)
    if guided is None:
        np.testing.assert_allclose(got, c, rtol=0, atol=1e-13 * mc.max())
        np.testing.assert_allclose(tol, (9 * C + 2) * 2.0 ** -24 * mc, rtol=1e-12)
        return
    s = float(np.float32(a["scale"]))
    if guided == "cfg":
        u, mu = (v.numpy() for v in _conv64(_rearranged(a["dec"][B * L:], B, L, e, C, P, S), a["wconv"], a["bconv"], C))
    else:
        u, mu = (v.numpy() for v in _conv64(_rearranged(a["dec2"], B, a["L2"], a["extras2"], C, P, S), a["wconv2"], a["bconv2"], C))
        assert a["extras2"] != e
    np.testing.assert_allclose(got, c + s * (c - u), rtol=0, atol=1e-13 * (mc.max() + mu.max()) * (1 + abs(s)))
    lin = (9 * C + 2) * 2.0 ** -24 * ((1 + abs(s)) * mc + abs(s) * mu)
    assert (tol >= lin).all() and (tol <= 1.2 * lin + 2.0 ** -22 * (np.abs(got) + abs(s) * np.abs(c - u))).all()


def test_philox4x32_10_known_answers():
    """the published Random123 vectors of philox4x32_10 (kat_vectors)"""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, want in kat:
        assert tuple(int(v) for v in ks.philox4x32_10(np.array(ctr, np.uint32), np.array(key, np.uint32))) == want
    got = ks.philox4x32_10(np.array([k[0] for k in kat], np.uint32), np.array([k[1] for k in kat], np.uint32))      # vectorised, a key per row
    assert got.dtype == np.uint32 and np.array_equal(got, np.array([k[2] for k in kat], np.uint32))


def test_philox_normal4_ref_against_a_scalar_box_muller():
    """the words of counter and key (a 64-bit id and a 64-bit seed use both halves), the float32 uniforms, and the float64 functions"""
    seed, ctr = (0xDEADBEEF << 32) | 0x12345678, 941
    pix = np.array([0, 1, 4095, (1 << 32) + 7, (5 << 32) | 0xFFFFFFFF], np.uint64)
    for stream in (ks.PHILOX_STEP, ks.PHILOX_KNOWN):
        z, ulog = ks.philox_normal4_ref(seed, pix, ctr, stream)
        assert z.shape == (5, 4) and z.dtype == np.float64 and ulog.dtype == np.float32
        for i, p in enumerate(int(v) for v in pix):
            c = [int(v) for v in ks.philox4x32_10(np.array([p & 0xFFFFFFFF, p >> 32, ctr, stream], np.uint32),
                                                  np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint32))]
            f = [torch.tensor(v, dtype=torch.int64).to(torch.float32) for v in c]                  # int -> float32, round to nearest even
            sc = torch.tensor(2.0 ** -32, dtype=torch.float32)
            for j in (0, 2):
                u = float((f[j] + 1.0) * sc)
                ang = float(torch.tensor(6.283185307179586, dtype=torch.float32) * (f[j + 1] * sc))
                r = math.sqrt(-2.0 * math.log(u))
                assert ulog[i, j // 2] == np.float32(u)
                assert abs(z[i, j] - r * math.cos(ang)) <= 1e-14 and abs(z[i, j + 1] - r * math.sin(ang)) <= 1e-14
    assert not np.array_equal(ks.philox_normal4_ref(seed, pix, ctr)[0], ks.philox_normal4_ref(seed, pix, ctr, ks.PHILOX_KNOWN)[0])
    # uint32 -> float32 rounds to nearest even: 2^32 - 129 is a tie between 2^32 - 256 and 2^32, and the even neighbour is 2^32
    assert np.uint32(0xFFFFFF7F).astype(np.float32) == np.float32(2.0 ** 32 - 256) and np.uint32(0xFFFFFF80).astype(np.float32) == np.float32(2.0 ** 32)
    zz = ks.philox_normal4_ref(3, np.arange(1 << 16, dtype=np.uint64), 0)[0]
    assert abs(zz.mean()) < 0.01 and abs(zz.std() - 1.0) < 0.01 and np.isfinite(zz).all()
    ids = ks.final_pixel_ids(2, 4, 5)
    assert ids.shape == (2, 4, 4) and int(ids[1, 2, 3]) == ((1 + 5) * 4 + 2) * 4 + 3 and int(ks.final_pixel_ids(2, 4, 5, True)[1, 2, 3]) == ((1 + 5) * 4 + 3) * 4 + 2
    assert int(ks.final_pixel_ids(1, 64, (1 << 20) + 5)[0, 0, 0]) == ((1 << 20) + 5) * 4096 > 1 << 32


def _r32(v):
    """a Python float (exact: sums and products of two float32 of nearby exponents fit float64) rounded to float32"""
    return float(np.float32(v))


def test_step_restatement_rounds_every_operation_once():
    r = np.random.default_rng(8)
    x, e, z, h, x0, z2 = (r.standard_normal(512).astype(np.float32) for _ in range(6))
    m = r.choice(np.array([0.0, 1.0, 0.25, 0.7], np.float32), 512)
    a, b, c, d, p, q, ka, kb = (float(np.float32(v)) for v in (0.9731, -0.2173, 0.3337, 0.1291, 1.0413, -0.3127, 0.8125, 0.5829))
    X, E, Z, H, X0, Z2, M = ([float(v) for v in arr] for arr in (x, e, z, h, x0, z2, m))
    f = lambda v: np.array(v, np.float32)
    want = [_r32(_r32(a * _r32(xi - _r32(b * ei))) + _r32(c * zi)) for xi, ei, zi in zip(X, E, Z)]
    assert np.array_equal(ks.step_ddpm(x, e, z, a, b, c), f(want))
    assert np.array_equal(ks.step_ddpm(x, e, None, a, b, c), f([_r32(a * _r32(xi - _r32(b * ei))) for xi, ei in zip(X, E)]))
    ab = [_r32(_r32(a * xi) + _r32(b * ei)) for xi, ei in zip(X, E)]
    abd = [_r32(v + _r32(d * hi)) for v, hi in zip(ab, H)]
    assert np.array_equal(ks.step_table(x, e, None, h, a, b, c, d, 0), f(ab))
    assert np.array_equal(ks.step_table(x, e, None, np.full(512, np.nan, np.float32), a, b, c, d, 0), f(ab)), "h must not enter without hist"
    assert np.array_equal(ks.step_table(x, e, z, h, a, b, c, d, 1), f([_r32(v + _r32(c * zi)) for v, zi in zip(abd, Z)]))
    assert np.array_equal(ks.step_table(x, e, z, h, a, b, c, d, 0), f([_r32(v + _r32(c * zi)) for v, zi in zip(ab, Z)]))
    assert np.array_equal(ks.step_history(x, e, p, q), f([_r32(_r32(p * xi) + _r32(q * ei)) for xi, ei in zip(X, E)]))
    # an FMA would differ: some element of a x + b e must change when the product is not rounded on its own
    assert any(_r32(a * xi + _r32(b * ei)) != v for xi, ei, v in zip(X, E, ab))
    xp = np.array(abd, np.float32)
    for use_z2, kbv in ((True, kb), (False, kb), (True, 0.0)):
        kn = [_r32(ka * v) if not use_z2 or kbv == 0.0 else _r32(_r32(ka * v) + _r32(kbv * w)) for v, w in zip(X0, Z2)]
        want = [xi if mi == 0.0 else _r32(_r32(mi * k) + _r32(_r32(1.0 - mi) * xi)) for xi, k, mi in zip(abd, kn, M)]
        x0n = np.where(m == 0, np.float32(np.nan), x0)                   # NaN in the known image wherever the mask is 0
        got = ks.step_known(xp, x0n, m, ka, kbv, z2 if use_z2 else None)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), f(want).view(np.uint32))
    assert np.array_equal(ks.step_known(xp, x0, np.zeros(512, np.float32), ka, kb, z2).view(np.uint32), xp.view(np.uint32))
    # float64: the same expressions without the float32 roundings
    assert np.array_equal(ks.step_table(x, e, z, h, a, b, c, d, 1, np.float64), a * x.astype(np.float64) + b * e.astype(np.float64) + d * h.astype(np.float64) + c * z.astype(np.float64))


MUTANTS = [(C, P, S, mut, guided) for C, P in ks.FINAL_FORMS for S in ks.FINAL_SIZES
           for mut, guided in (("taps", None), ("chan_first", None), ("edge_shift", "cfg"), ("same_weights", "auto"))
           if not (mut == "chan_first" and (C == 1 or P == 1)) and not (mut == "edge_shift" and S <= 16)]


@pytest.mark.parametrize("C,P,S,mut,guided", MUTANTS)
def test_a_mutant_head_exceeds_the_bound_on_the_test_inputs(C, P, S, mut, guided):
    """the reference with one deliberate error, against the bound the kernel is held to, on the inputs tests/test_final_step.py uses"""
    a = ks.final_head_inputs(C, P, S, guided)
    want, tol = ks.final_eps64(**a)
    bad, _ = ks.final_eps64(**a, mutant=mut)
    over = np.abs(bad - want) > tol
    if mut == "edge_shift":                   # only the last column of a tile that has a right-hand neighbour reads the shifted halo
        hit = np.zeros(S, bool)
        hit[15:S - 1:16] = True
        assert hit.any() and not over[..., ~hit].any() and np.array_equal(bad[..., ~hit], want[..., ~hit])
        assert over[..., hit].mean() > 0.9
    else:
        assert over.mean() > 0.9, over.mean()


@pytest.mark.parametrize("case", ks.PHILOX_CASES, ids=lambda c: f"S{c['S']}-C{c['C']}-b{c['b0']}-k{c['ctr']}-{'z2' if c['z2'] else 'z'}")
def test_philox_cases_near_one_cap_and_the_transposed_id(case):
    """at most 1 % of a case's draws may be judged at the looser bound of log near 0; the pixel id built as x S + y is off by order 1"""
    stream = ks.PHILOX_KNOWN if case["z2"] else ks.PHILOX_STEP
    z, near = ks.final_philox_ref(case["seed"], case["B"], case["C"], case["S"], case["b0"], case["ctr"], stream)
    assert z.shape == near.shape == (case["B"], case["C"], case["S"], case["S"]) and np.isfinite(z).all()
    assert near.mean() <= 0.01, near.mean()
    bad, _ = ks.final_philox_ref(case["seed"], case["B"], case["C"], case["S"], case["b0"], case["ctr"], stream, transposed=True)
    diag = np.eye(case["S"], dtype=bool)
    assert np.array_equal(bad[..., diag], z[..., diag]) and (np.abs(bad - z)[..., ~diag] > 1e-4).mean() > 0.99
    # every other mix-up the test exists for: the other stream word, counter, seed half, image
    for other in (ks.final_philox_ref(case["seed"], case["B"], case["C"], case["S"], case["b0"], case["ctr"], stream ^ 1)[0],
                  ks.final_philox_ref(case["seed"], case["B"], case["C"], case["S"], case["b0"], case["ctr"] + 1, stream)[0],
                  ks.final_philox_ref(case["seed"] ^ (1 << 32), case["B"], case["C"], case["S"], case["b0"], case["ctr"], stream)[0],
                  ks.final_philox_ref(case["seed"], case["B"], case["C"], case["S"], case["b0"] + 1, case["ctr"], stream)[0],
                  ks.final_philox_ref(case["seed"], case["B"], case["C"], case["S"], case["b0"] & 0xFFFFF, case["ctr"], stream)[0]
                  if case["b0"] >> 20 else None):
        assert other is None or (np.abs(other - z) > 1e-4).mean() > 0.99


# ---------------------------------------------------------------------------------------------------------------- the KL-VAE kernels
# The references of tests/test_vae_kernels.py against torch in float64, and -- on the very inputs the GPU tests use -- every deliberate error
# against the bound (or the bit equality) the kernel is held to.
@pytest.mark.parametrize("C", ks.GATHER_C)
@pytest.mark.parametrize("kind,B,H,W", ks.GATHER_SHAPES)
def test_im2col_reference_against_unfold_and_its_mutants(kind, B, H, W, C):
    import torch.nn.functional as TF
    src = ks.gather_input(kind, B, H, W, C)
    assert np.array_equal(bf16(src), src) and src.shape == (B, H // (2 if kind == 3 else 1), W // (2 if kind == 3 else 1), C)
    kpad = ks.vae_kpad(C, "bf16")
    assert kpad % 64 == 0 and 9 * C <= kpad < 9 * C + 64 and ks.vae_kpad(C, "fp32") % 32 == 0
    want = ks.im2col3x3_ref(src, kind == 3, kpad)
    t = torch.from_numpy(src).permute(0, 3, 1, 2)
    if kind == 3:
        t = TF.interpolate(t, scale_factor=2.0, mode="nearest")
    cols = TF.unfold(t, 3, padding=1).reshape(B, C, 3, 3, H * W).permute(0, 4, 2, 3, 1).reshape(B * H * W, 9 * C).numpy()
    assert np.array_equal(want[:, :9 * C], cols) and not want[:, 9 * C:].any()
    muts = ["edge"] + (["taps"] if H * W > 1 else []) + (["half_x"] if kind == 3 and W > 2 else [])      # (one source column: nothing to halve)
    for mut in muts:
        bad = ks.im2col3x3_ref(src, kind == 3, kpad, mutant=mut)
        assert (bad != want).any(1).mean() >= 0.5, mut      # at least half of the rows differ (a 2 x 2 upsample of one pixel: the diagonal agrees)


@pytest.mark.parametrize("swish", [0, 1])
@pytest.mark.parametrize("B,HW,C", ks.GN_SHAPES)
def test_groupnorm_reference_and_its_mutants(B, HW, C, swish):
    """the numpy restatement equals torch's float64 group_norm; each mutant, and the emulation of the one-pass fp32 statistics, exceeds the
    fp32 bound of tests/test_vae_kernels.py; the emulation of the statistics about a per-(image, group) pivot stays within it"""
    case = ks.gn_case(B, HW, C, swish)
    x, gamma, beta, want = case["x"], case["gamma"], case["beta"], case["want"]
    assert np.abs(ks.groupnorm_ref(x, gamma, beta, B, HW, C, swish) - want).max() < 1e-11
    tol = ks.gn_tol(case, "fp32")
    assert (case["e32"] > 0).all() and case["e32"].max() == case["e32_case"] and tol.max() < 1e-3
    if B > 1:      # the pairs rotate with the image
        k = ks.gn_pair_index(B, C)
        assert (k[0] != k[1]).all() and set(k[0]) == {0, 1, 2, 3}
    if C != 128:
        assert (np.abs(ks.groupnorm_ref(x, gamma, beta, B, HW, C, swish, mutant="group_map") - want) > tol).mean() > 0.5
    else:
        assert np.array_equal(ks.groupnorm_ref(x, gamma, beta, B, HW, C, swish, mutant="group_map"), ks.groupnorm_ref(x, gamma, beta, B, HW, C, swish))
    if HW > 256 and HW % 256:
        assert (np.abs(ks.groupnorm_ref(x, gamma, beta, B, HW, C, swish, mutant="drop_tail") - want) > tol).mean() > 0.5
    one = np.abs(ks.groupnorm_emulated(x, gamma, beta, B, HW, C, swish, pivot=False) - want)
    piv = np.abs(ks.groupnorm_emulated(x, gamma, beta, B, HW, C, swish, pivot=True) - want)
    ratio = lambda e: [float((e / case["e32"])[case["cls"] == k].max()) for k in range(4)]
    print(f"B {B} HW {HW} C {C} swish {swish}: err / e32 per (mean, std) pair, one-pass {ratio(one)}, about a pivot {ratio(piv)}")
    assert (piv <= tol).all()
    r = ratio(one)
    assert r[0] <= 8 and r[1] > 8 and r[2] > 80 and r[3] > 80, r
    assert one.max() > 8 * case["e32_case"]                # it fails the bound taken over the whole case, too


def test_groupnorm_constant_case():
    case = ks.gn_case(2, 64, 128, 0, const=True)
    x = case["x"].reshape(2, 64, 128)
    assert (x[0, :, 28:32] == np.float32(123.456)).all() and (x[1, :, 20:24] == np.float32(0.1)).all()
    assert np.abs(case["want"].reshape(2, 64, 128)[1, :, 20:24] - case["beta"][20:24]).max() < 1e-9
    assert (np.abs(ks.groupnorm_emulated(case["x"], case["gamma"], case["beta"], 2, 64, 128, 0, pivot=True) - case["want"]) <= ks.gn_tol(case, "fp32")).all()


@pytest.mark.parametrize("rows,n", ks.SOFTMAX_SHAPES)
def test_softmax_reference_and_its_mutants(rows, n):
    s = ks.softmax_inputs(rows, n)
    want, tol = ks.softmax_ref(s, ks.SOFTMAX_SCALE)
    t = torch.softmax(torch.from_numpy(s).double() * float(ks.SOFTMAX_SCALE), dim=-1).numpy()
    assert np.abs(want - t).max() < 1e-14 and np.abs(want.sum(-1) - 1).max() < 1e-12
    assert tol.max() < 1e-4 and (tol >= 2.0 ** -126).all()
    a = s.astype(np.float64) * float(ks.SOFTMAX_SCALE)
    if rows >= 4 and n > 1:
        assert a[3].max() > 79.9 and a[3].min() < -79.9 and (s[2] == s[2, 0]).all() and want[1, -1] == 1.0
    if n > 1:
        assert (np.abs(ks.softmax_ref(s, ks.SOFTMAX_SCALE, mutant="no_scale")[0] - want) > tol).any(1)[np.isin(np.arange(rows) % 4, (0, 3))].all()      # (a constant or a one-hot row stays what it is)
    if n % 64:
        bad = ks.softmax_ref(s, ks.SOFTMAX_SCALE, mutant="drop_tail")[0]
        over = ~(np.abs(bad - want) <= tol)
        assert over.any(1)[np.arange(rows) % 4 != 3 if n > 64 else slice(None)].all()
    # bf16: the bound grows by one ulp of the result
    assert np.array_equal(ks.softmax_ref(s, ks.SOFTMAX_SCALE, "bf16")[1], tol + ulp_bf16(want))


@pytest.mark.parametrize("B,HW", ks.VAE_MOMENTS_SHAPES)
def test_moments_reference_and_its_mutants(B, HW):
    import torch.nn.functional as TF
    a = ks.vae_moments_case(B, HW)
    m, tol_m, z, tol_z = ks.vae_moments_ref(a["h"], a["w"], a["b"], a["eps"], B, HW)
    hh = torch.from_numpy(a["h"]).double().reshape(B, HW, 8).permute(0, 2, 1).reshape(B, 8, HW, 1)
    mt = TF.conv2d(hh, torch.from_numpy(a["w"]).double().reshape(8, 8, 1, 1), torch.from_numpy(a["b"]).double()).reshape(B, 8, HW)
    assert np.abs(m - mt.numpy()).max() < 1e-12
    mean, lv = mt[:, :4], torch.clamp(mt[:, 4:], -30.0, 20.0)
    zt = float(np.float32(ks.VAE_SCALE)) * (mean + torch.exp(0.5 * lv) * torch.from_numpy(a["eps"]).double())
    assert (np.abs(z - zt.numpy()) <= 1e-12 * (1 + np.abs(z))).all()
    lvr = m[:, 4:]
    assert (lvr < -30).any() and (lvr > 20).any() and ((lvr > -30) & (lvr < 20)).any()
    mode = ks.vae_moments_ref(a["h"], a["w"], a["b"], None, B, HW)
    assert np.array_equal(mode[2], float(np.float32(ks.VAE_SCALE)) * m[:, :4]) and (mode[3] <= tol_z).all()
    mw = ks.vae_moments_ref(a["h"], a["w"], a["b"], a["eps"], B, HW, mutant="w_transposed")
    assert (np.abs(mw[0] - m) > tol_m).mean() > 0.9 and (np.abs(mw[2] - z) > tol_z).mean() > 0.9
    nc = ks.vae_moments_ref(a["h"], a["w"], a["b"], a["eps"], B, HW, mutant="no_clamp")
    assert np.array_equal(nc[0], m) and (np.abs(nc[2] - z) > tol_z)[lvr > 20.01].all() and np.array_equal(nc[2][np.abs(lvr + 5) < 25], z[np.abs(lvr + 5) < 25])
    lm = ks.vae_moments_ref(a["h"], a["w"], a["b"], a["eps"], B, HW, mutant="logvar_from_mean")
    assert np.array_equal(lm[0], m) and (np.abs(lm[2] - z) > tol_z).mean() > 0.9


@pytest.mark.parametrize("B,HW", ks.VAE_INPUT_SHAPES)
def test_vae_input_reference_and_its_mutant(B, HW):
    a = ks.vae_input_case(B, HW)
    want, tol = ks.vae_input_ref(a["z"], a["w"], a["b"], a["inv_scale"])
    zz = torch.from_numpy(a["z"]).double() * float(a["inv_scale"])
    t = torch.einsum("oc,bcp->bpo", torch.from_numpy(a["w"]).double(), zz) + torch.from_numpy(a["b"]).double()
    assert np.abs(want - t.reshape(B * HW, 4).numpy()).max() < 1e-13 and tol.max() < 1e-4
    assert (np.abs(ks.vae_input_ref(a["z"], a["w"], a["b"], a["inv_scale"], mutant="w_transposed")[0] - want) > tol).mean() > 0.9
    # the fp32 restatement of the chain lies within the bound
    v = (a["z"].transpose(0, 2, 1).reshape(-1, 4) * a["inv_scale"]).astype(np.float32)
    acc = np.broadcast_to(a["b"], (B * HW, 4)).astype(np.float32)
    for c in range(4):
        acc = (acc.astype(np.float64) + a["w"][:, c].astype(np.float64) * v[:, c:c + 1].astype(np.float64)).astype(np.float32)      # an fmaf: one rounding
    assert (np.abs(acc - want) <= tol).all()


def test_vae_output_reference_and_cast_inputs():
    inp = np.arange(2 * 5 * 4, dtype=np.float32).reshape(10, 4)
    out = ks.vae_output_ref(inp, 2, 3, 5, 4)
    assert out.shape == (2, 3, 5) and all(out[b, c, p] == inp[b * 5 + p, c] for b in range(2) for c in range(3) for p in range(5))
    x = ks.cast_inputs()
    u = x.view(np.uint32)
    tie = (u & 0xFFFF) == 0x8000
    up, down = tie & ((u >> 16) & 1 == 1), tie & ((u >> 16) & 1 == 0)
    assert x.size % 256 and up.sum() >= 512 and down.sum() >= 512 and (x[tie] < 0).any() and (x[tie] > 0).any()
    assert np.array_equal(bf16_bits(x[up]), (u[up] >> 16) + 1) and np.array_equal(bf16_bits(x[down]), u[down] >> 16)
    assert (u == 0).any() and (u == 0x80000000).any()
    mag = np.abs(x[x != 0])
    assert mag.min() < 2.0 ** -19 and mag.max() > 2.0 ** 19


# ---------------------------------------------------------------------------------------------------------------- the early-exit probes
@pytest.mark.parametrize("D,L", ks.EE_PROBE_CASES)
def test_probe_rows_reference_and_its_mutants(D, L):
    """the inputs of tests/test_ee_probes.py: the reference is torch's float64 Linear + Sigmoid + mean, the float32 restatement of the kernel
    lies within the bound, every mutant of the rows and of the mean lies outside it"""
    B = ks.EE_B
    a = ks.ee_probe_case(B, L, D)
    s, tol_s = ks.probe_rows_ref(a["x"], a["w"], a["b"])
    lin = torch.nn.Linear(D, 1).double()
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(a["w"]).double()[None])
        lin.bias.fill_(float(a["b"]))
        st = torch.sigmoid(lin(torch.from_numpy(a["x"]).double())).squeeze(-1)
    assert np.abs(s - st.numpy()).max() < 1e-13 and tol_s.max() < 1e-3 and (tol_s >= ks.FLOOR).all()      # (the largest: the offset rows)
    out, tol = ks.probe_mean_ref(s, tol_s)
    assert np.abs(out - st.mean(1).numpy()).max() < 1e-14 and tol.max() < 2e-4
    # what the inputs cover: logits within a few units, of +-30, saturated either way, below 2^-126, and the offset rows' cancellation
    logit = a["x"].astype(np.float64) @ a["w"].astype(np.float64) + 0.7
    mag = np.abs(a["x"].astype(np.float64)) @ np.abs(a["w"].astype(np.float64))
    assert (np.abs(logit) < 3).any() and abs(float(a["w"].astype(np.float64).sum()) - 0.02) < 1e-6
    if L >= 9:
        assert (np.abs(logit) > 20).any() and (logit > 90).any() and (logit < -90).any() and ((s < ks.FLOOR) & (s > 0)).any()
        assert (mag > 50 * np.sqrt(D))[np.abs(logit) < 8].any()
    # the float32 restatement of the kernel, and of the reduce on its rows (against the float64 rows and against its own)
    s32 = ks.probe_rows_f32(a["x"], a["w"], a["b"])
    assert gate(s32, s, tol_s, "float32 rows") <= 1.0
    m32 = ks.probe_mean_f32(s32)
    assert gate(m32, out, tol, "float32 mean of the float32 rows") <= 1.0
    assert gate(m32, *ks.probe_mean_ref(s32), "float32 mean against its own rows") <= 1.0
    # the row mutants: out of bound in the rows and in the mean, of image 0 at least
    per = -(-L // 8)
    for mut in ks.EE_ROW_MUTANTS:
        if mut == "pair_repeats" and per < 5:      # (slices of fewer than five rows have no second row in flight)
            assert np.array_equal(ks.probe_rows_ref(a["x"], a["w"], a["b"], mutant=mut)[0], s)
            continue
        bad = ks.probe_rows_ref(a["x"], a["w"], a["b"], mutant=mut)[0]
        assert (np.abs(bad - s) > tol_s)[0].any(), mut
        assert (np.abs(bad.mean(-1) - out) > tol)[0], mut
    for mut in ks.EE_MEAN_MUTANTS:
        if mut == "drop_tail" and L % 64 == 0:
            continue
        bad = ks.probe_mean_ref(s, tol_s, mutant=mut)[0]
        assert (~(np.abs(bad - out) <= tol))[0], mut      # (at L = 1 image 2 is one row below 2^-126: nothing to drop)


def test_probe_row_selection_reference():
    """the per-timestep table of test_ee_probe_selects_its_row_from_the_step_state: only the selected row is finite, so the row `add` is NaN"""
    D, L, t_mul, add = 512, 17, 4, 2
    for t in (0, 3, 6):
        a = ks.ee_probe_case(ks.EE_B, L, D, n_probe=7 * 4, row=t * t_mul + add)
        s, tol_s = ks.probe_rows_ref(a["x"], a["pw"], a["pb"], row=t * t_mul + add)
        assert np.array_equal(s, ks.probe_rows_ref(a["x"], a["w"], a["b"])[0]) and np.isfinite(s).all()
        assert np.isnan(a["pw"]).all(1).sum() == 27 and np.isnan(a["pb"]).sum() == 27
        if t:
            bad = ks.probe_rows_ref(a["x"], a["pw"], a["pb"], row=t * t_mul + add, mutant="wrong_probe_row", wrong_row=add)[0]
            with pytest.raises(AssertionError):
                gate(bad, s, tol_s, "row `add` of the table")


@pytest.mark.parametrize("L", ks.EE_REDUCE_L)
@pytest.mark.parametrize("rows", ks.EE_REDUCE_ROWS)
def test_probe_reduce_emulation_and_its_mutants(rows, L):
    s = ks.ee_reduce_rows(rows, L)
    assert s.min() >= 0 and s.max() <= 1 and (L == 1 or (s == 1).any()) and not ((s > 0) & (s < ks.FLOOR)).any()
    out, tol = ks.probe_mean_ref(s)
    assert np.abs(out - torch.from_numpy(s).double().mean(1).numpy()).max() < 1e-15 and (out > 0).all()
    emu = ks.probe_mean_f32(s)
    assert emu.dtype == np.float32 and gate(emu, out, tol, "the float32 emulation") <= 1.0
    # the emulation's order, spelled out for one row with scalars
    acc = [np.float32(0)] * 64
    for l in range(L):
        acc[l % 64] = np.float32(acc[l % 64] + s[0, l])
    for o in (32, 16, 8, 4, 2, 1):
        acc = [np.float32(acc[i] + acc[i ^ o]) for i in range(64)]
    assert np.float32(acc[0] / np.float32(L)) == emu[0]
    for mut in ks.EE_MEAN_MUTANTS:
        if mut == "drop_tail" and L % 64 == 0:
            continue
        assert (~(np.abs(ks.probe_mean_ref(s, mutant=mut)[0] - out) <= tol)).all(), mut


@pytest.mark.parametrize("D,L", ks.EE_ATTN_CASES)
def test_attn_probe_reference_and_its_mutants(D, L):
    import torch.nn.functional as TF
    B = ks.EE_B
    a = ks.ee_attn_case(B, L, D)
    ops = [a[k] for k in ("x", "q", "wkv", "bkv", "w0", "b0", "w2", "b2")]
    out, tol = ks.attn_probe_ref(*ops)
    # models/early_exit.py AttentionProbe.forward in float64: scaled_dot_product_attention of the learned query, then the Sequential
    t = {k: torch.from_numpy(v).double() for k, v in a.items() if isinstance(v, np.ndarray)}
    kv = TF.linear(t["x"][:, 1:], t["wkv"], t["bkv"])
    k_, v_ = kv[..., :D][:, None], kv[..., D:][:, None]                    # [B, 1 head, n, D]
    att = TF.scaled_dot_product_attention(t["q"].reshape(1, 1, 1, D).expand(B, 1, 1, D), k_, v_).reshape(B, D)
    seq = torch.nn.Sequential(torch.nn.Linear(D, D), torch.nn.SiLU(), torch.nn.Linear(D, 1)).double()
    with torch.no_grad():
        seq[0].weight.copy_(t["w0"]); seq[0].bias.copy_(t["b0"]); seq[2].weight.copy_(t["w2"][None]); seq[2].bias.copy_(t["b2"])
        want = seq(att).squeeze(-1).numpy()
    assert (np.abs(out - want) <= 1e-9 * (1 + np.abs(want))).all()
    assert (tol[:2] < 1e-2).all() and tol[2] < 0.5      # (image 2: scores near 1e3 carry fp32 errors near 1e-3)
    # what the inputs hold: bk's constant is large; token 0 would take the softmax over; the last token carries weight; image 1 is one-hot
    u = a["wkv"][:D].astype(np.float64).T @ a["q"].astype(np.float64) / np.sqrt(D)
    sc = a["x"].astype(np.float64) @ u
    assert abs(float(a["bkv"][:D].astype(np.float64) @ a["q"].astype(np.float64))) / np.sqrt(D) > 0.5
    assert (sc[:, 0] - sc[:, 1:].max(-1))[[0, 2]].min() > 29 and sc[2, 1:].min() > 900
    if L > 2:
        assert (sc[1, -1] - sc[1, 1:-1].max()) > 100
        p0 = np.exp(sc[0, 1:] - sc[0, 1:].max())
        assert p0[-1] / p0.sum() > 2.0 / L
    # the float32 restatement of the folded form lies within the bound
    assert gate(ks.attn_probe_f32(*ops), out, tol, "float32 evaluation of the folded form") <= 1.0
    for mut in ks.EE_ATTN_MUTANTS:
        bad = ks.attn_probe_ref(*ops, mutant=mut)[0]
        if (mut == "drop_far_tokens" and L <= 257) or (mut == "no_scale" and L == 2):      # (no token behind index 256; one token: p = 1)
            assert np.array_equal(bad, out)
            continue
        over = np.abs(bad - out) > tol
        assert over[1 if mut == "drop_far_tokens" else 0], (mut, np.abs(bad - out) / tol)
