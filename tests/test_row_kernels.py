"""GPU unit tests of the row kernels every forward pass starts with (csrc/rowops.hip): layernorm_kernel<T> row-major and in fragment order,
embed_kernel and embed_mfma_kernel<4,3> / <2,3> / <2,4> / <4,3,512> (token assembly, the last one with the first block's norm1), time_mlp_kernel
-- each through its development entry point (include/duodiff_dev.h dd_dev_layernorm / dd_dev_embed / dd_dev_time_mlp) against float64.
Replaces reference models/uvit.py:221-225, 95-115, 264-272, 352-365 and nn.LayerNorm.

Gates (per element; every e32 is the error of a numpy-float32 evaluation of the same formula against float64, computed here for the case):
  * LayerNorm, fp32 out: max(4 e32, 2e-6).  e32 tracks (4 + |mean| / sigma) 2^-23: 9e-7 for centred rows, 9e-4 at offset 2000 / sigma 0.5
    (for the 1- and 5-row cases it is taken over the 516-row set they are cut from: ln_tolerances).
    bf16 out (row-major and fragment order): 2^-8 |want| + 2 x the fp32 bound of the case.
  * embed, patch and label columns: (pd + 2) 2^-24 (sum_k |w_k x_k| + |bias| + |pos|), the running-error bound of a length-pd fp32 sum;
    time-token columns: 2^-18 max(1, |t f|), twice the estimate from fp32 expf of the frequency and the rounding of the argument.
  * time_embed MLP: max(8 e32, 1e-6 max |want|); the float32 evaluation starts from t as the kernel does (the fp32 sinusoid's argument
    error at t = 999 is part of any fp32 evaluation of the formula).
Exact: canary rows untouched, padding rows zero, rows a launch does not own bit-unchanged, x_tok of the norm1 variant bit-equal to the plain one.
test_gates_reject_the_bugs_they_are_meant_to_catch (CPU, no GPU mark) feeds corrupted references to the same gates.
"""
import ctypes as C

import numpy as np
import pytest

import kernel_support
from kernel_support import NAN16, NAN32, PREC_BF16, PREC_FP32, P, bf16, from_bf16_bits, gate, round_up, to_frag, unfrag

gpu = pytest.mark.gpu

LN_OFFSETS = [(0.0, 1.0), (100.0, 1.0), (-1000.0, 2.0), (2000.0, 0.5)]


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
def ln_ref(x, g, b, dtype=np.float64):
    """two-pass LayerNorm (eps 1e-5, biased variance) in `dtype`"""
    x, g, b = (np.asarray(a, dtype) for a in (x, g, b))
    mean = x.mean(-1, keepdims=True, dtype=dtype)
    d = x - mean
    var = (d * d).mean(-1, keepdims=True, dtype=dtype)
    return d * (dtype(1) / np.sqrt(var + dtype(1e-5))) * g + b


def ln_tolerances(x, g, b, x_many=None):
    """(want, fp32 bound, bf16 bound) of fp32 rows x.  x_many: more rows of the same offset and sigma.  The float32 evaluation's error of ONE row is
    mostly the rounding of that row's mean, anything between 0 and its largest value: a sample of one.  e32 of a case of few rows is therefore
    the larger of its own rows' and of the 516-row set's of the same D, offset and sigma."""
    want = ln_ref(x, g, b)
    e32 = float(np.abs(ln_ref(x, g, b, np.float32).astype(np.float64) - want).max())
    if x_many is not None:
        e32 = max(e32, float(np.abs(ln_ref(x_many, g, b, np.float32).astype(np.float64) - ln_ref(x_many, g, b)).max()))
    t32 = max(4.0 * e32, 2e-6)
    return want, t32, 2.0 ** -8 * np.abs(want) + 2.0 * t32


def ln_rows(rows, D, offset, sigma, seed):
    r = np.random.default_rng(seed)
    x = (offset + sigma * r.standard_normal((rows, D))).astype(np.float32)
    g = (1.0 + 0.2 * r.standard_normal(D)).astype(np.float32)
    b = (0.3 * r.standard_normal(D)).astype(np.float32)
    return x, g, b


def run_layernorm(prec, x, g, b, frag=False, tok=(0, 0)):
    """dd_dev_layernorm; returns (status, out [rows + 8, D] as stored, frag [rows + 8, D] bf16 bits or None)"""
    ctx = kernel_support.ctx()
    rows, D = x.shape
    out = np.full((rows + 8, D), 0xA5A5 if prec == PREC_BF16 else 0xA5A5A5A5, np.uint16 if prec == PREC_BF16 else np.uint32)
    fr = np.full((rows + 8, D), 0xA5A5, np.uint16) if frag else None
    gb = np.ascontiguousarray(np.stack([g, b]), np.float32)
    st = ctx.lib.dd_dev_layernorm(ctx.handle, prec, rows, D, P(np.ascontiguousarray(x)), P(gb), P(out), P(fr), tok[0], tok[1], 0, None,
                                  C.byref(C.c_float(0)))
    return st, out, fr


@gpu
@pytest.mark.parametrize("D", [64, 128, 192, 256, 512, 768, 1024])
@pytest.mark.parametrize("prec", [PREC_BF16, PREC_FP32], ids=["bf16", "fp32"])
def test_layernorm_against_float64_reference(prec, D):
    """the scalar path (D % 256 != 0) and the vector path; 1 row, 5 rows and 516 = 129 workgroups of 4 (5: a ragged last workgroup); rows with
    a large common offset"""
    for offset, sigma in LN_OFFSETS:
        x_many, g, b = ln_rows(516, D, offset, sigma, seed=D)
        for rows in (516, 5, 1):
            x = x_many[516 - rows:]
            want, t32, t16 = ln_tolerances(x, g, b, x_many)
            st, out, _ = run_layernorm(prec, x, g, b)
            kernel_support.ctx().check(st)
            assert np.all(out[rows:] == (NAN16 if prec == PREC_BF16 else NAN32)), "the rows behind the output were written"
            got = from_bf16_bits(out[:rows]) if prec == PREC_BF16 else out[:rows].view(np.float32)
            what = f"layernorm {'bf16' if prec == PREC_BF16 else 'fp32'} D={D} rows={rows} offset={offset} sigma={sigma}"
            ratio = gate(got, want, t16 if prec == PREC_BF16 else t32, what)
            print(f"{what}: error / bound {ratio:.3f} (fp32 bound {t32:.2e}, max |err| {np.abs(got - want).max():.2e})")


@gpu
@pytest.mark.parametrize("tok_l,tok_e", [(33, 1), (66, 2), (257, 1), (258, 2)])
@pytest.mark.parametrize("D", [256, 512, 768, 1024])
def test_layernorm_in_fragment_order(D, tok_l, tok_e):
    nimg = 3 if tok_l < 100 else 2
    rows, tok_n = nimg * tok_l, tok_l - tok_e
    for offset, sigma in LN_OFFSETS[:2]:
        x, g, b = ln_rows(rows, D, offset, sigma, seed=D + tok_l)
        want, _, t16 = ln_tolerances(x, g, b)
        st, out, fr = run_layernorm(PREC_BF16, x, g, b, frag=True, tok=(tok_l, tok_e))
        kernel_support.ctx().check(st)
        is_patch = (np.arange(rows) % tok_l) >= tok_e
        groups = nimg * tok_n // 32
        what = f"layernorm frag D={D} tok_l={tok_l} tok_e={tok_e} offset={offset}"
        r1 = gate(from_bf16_bits(unfrag(fr, groups, D)), want[is_patch], t16[is_patch], what + " patch rows")
        r2 = gate(from_bf16_bits(out[:rows][~is_patch]), want[~is_patch], t16[~is_patch], what + " extra-token rows")
        print(f"{what}: error / bound {r1:.3f} (patch rows, fragment order), {r2:.3f} (extra-token rows)")
        assert np.all(out[:rows][is_patch] == NAN16) and np.all(out[rows:] == NAN16), "patch rows of the row-major output were written"
        assert np.all(fr.reshape(-1)[groups * 32 * D:] == NAN16), "the fragment buffer was written past its last group"


@gpu
def test_layernorm_refuses_what_it_does_not_support():
    from duodiff_amd import _lib
    for prec in (PREC_BF16, PREC_FP32):
        for D in (96, 1088):
            x, g, b = ln_rows(8, D, 0.0, 1.0, 1)
            st, out, _ = run_layernorm(prec, x, g, b)
            assert st == _lib.DD_ERR_UNSUPPORTED and np.all(out.view(np.uint8) == 0xA5), (prec, D, st)
    for rows, D, tok in [(68, 256, (34, 1)), (70, 256, (33, 1)), (66, 128, (33, 1)), (66, 1280, (33, 1)), (66, 256, (2, 2))]:
        x, g, b = ln_rows(rows, D, 0.0, 1.0, 2)
        st, out, fr = run_layernorm(PREC_BF16, x, g, b, frag=True, tok=tok)
        assert st == _lib.DD_ERR_UNSUPPORTED and np.all(out == 0xA5A5) and np.all(fr == 0xA5A5), (rows, D, tok, st)
    x, g, b = ln_rows(66, 256, 0.0, 1.0, 3)
    st, _, _ = run_layernorm(PREC_FP32, x, g, b, frag=True, tok=(33, 1))      # fragment order is a bf16 output
    assert st == _lib.DD_ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------- token assembly
def sinusoid(t, D, normalize, dtype=np.float64):
    """timestep_embedding (models/uvit.py:95-115): [cos(t f_i) | sin(t f_i)], f_i = exp(-ln(1e4) i / half); returns (embedding [B, D], |t f| [B, D])"""
    half = D // 2
    t = np.asarray(t, dtype)
    tt = t / dtype(1000) if normalize else t
    f = np.exp((dtype(-np.log(10000.0)) * np.arange(half, dtype=dtype)) / dtype(half))
    arg = tt[:, None] * f[None]
    emb = np.concatenate([np.cos(arg), np.sin(arg)], -1)
    mag = np.concatenate([np.abs(arg), np.abs(arg)], -1)
    if D % 2:
        emb, mag = (np.concatenate([a, np.zeros_like(a[:, :1])], -1) for a in (emb, mag))
    return emb, mag


def embed_operands(B, C, S, Pz, D, extras, seed, num_classes=10):
    r = np.random.default_rng(seed)
    pd, L = C * Pz * Pz, extras + (S // Pz) ** 2
    x = r.standard_normal((B, C, S, S)).astype(np.float32)
    w = (r.standard_normal((D, C, Pz, Pz)) / np.sqrt(pd)).astype(np.float32)
    bias = (0.3 * r.standard_normal(D)).astype(np.float32)
    pos = (0.5 * r.standard_normal((L, D))).astype(np.float32)
    label = r.standard_normal((num_classes, D)).astype(np.float32)
    y = r.integers(0, num_classes, B).astype(np.int64)
    y[0] = num_classes - 1
    y[-1] = 0 if B > 1 else y[-1]
    return x, w, bias, pos, label, y


def embed_ref(x, w, bias, pos, label, y, t, extras, normalize, pos_shift=0):
    """float64 (want, tol) [B, L, D] of token assembly; pos_shift: the bug of an extra token that takes the pos_embed row of its neighbour"""
    B, C, S, _ = x.shape
    D, _, Pz, _ = w.shape
    g, pd = S // Pz, C * Pz * Pz
    L = extras + g * g
    patches = x.astype(np.float64).reshape(B, C, g, Pz, g, Pz).transpose(0, 2, 4, 1, 3, 5).reshape(B, g * g, pd)
    w2 = w.astype(np.float64).reshape(D, pd)
    p64, b64 = pos.astype(np.float64), bias.astype(np.float64)
    want, tol = np.zeros((B, L, D)), np.zeros((B, L, D))
    want[:, extras:] = patches @ w2.T + b64 + p64[extras:]
    tol[:, extras:] = (pd + 2) * 2.0 ** -24 * (np.abs(patches) @ np.abs(w2).T + np.abs(b64) + np.abs(p64[extras:]))
    emb, mag = sinusoid(t, D, normalize)
    want[:, extras - 1] = emb + p64[extras - 1 + pos_shift]
    tol[:, extras - 1] = 2.0 ** -18 * np.maximum(1.0, mag)
    if extras == 2:
        yy = np.clip(y, 0, label.shape[0] - 1)
        want[:, 0] = label.astype(np.float64)[yy] + p64[0 + pos_shift]
        tol[:, 0] = (pd + 2) * 2.0 ** -24 * (np.abs(label.astype(np.float64)[yy]) + np.abs(p64[0]))
    return want, tol


def run_embed(x, w, bias, pos, label, y, extras, normalize, generic, t_vec=None, t_state=0.0, ln=None):
    """dd_dev_embed; returns (x_tok [Mp + 8, D] fp32 as uint32 bits, ln_frag [Mp + 8, D] bf16 bits or None)"""
    ctx = kernel_support.ctx()
    B, Cn, S, _ = x.shape
    D, _, Pz, _ = w.shape
    L = extras + (S // Pz) ** 2
    Mp = round_up(B * L, 256)
    xt = np.full((Mp + 8, D), 0xA5A5A5A5, np.uint32)
    fr = np.full((Mp + 8, D), 0xA5A5, np.uint16) if ln is not None else None
    lnp = None if ln is None else np.ascontiguousarray(np.stack(ln), np.float32)
    tv = None if t_vec is None else np.ascontiguousarray(t_vec, np.float32)
    ctx.check(ctx.lib.dd_dev_embed(ctx.handle, B, Cn, S, Pz, D, extras, label.shape[0], int(normalize), int(generic), P(x), P(w), P(bias), P(pos),
                                   P(label) if extras == 2 else None, P(y) if extras == 2 else None, P(tv), float(t_state), P(lnp), P(xt), P(fr),
                                   0, None, C.byref(C.c_float(0))))
    return xt, fr


# (B, extras, normalize, per-row timesteps or None: the StepState's)
EMBED_MODES = {1: (1, 0, None, 999.0), 3: (2, 0, [0.0, 1.0, 999.0], 0.0), 9: (2, 1, [999.0, 0.0, 1.0, 500.0, 37.0, 998.0, 250.0, 3.0, 640.0], 0.0),
               17: (1, 1, None, 731.0), 2: (2, 0, None, 1.0), 5: (1, 0, [0.0, 999.0, 1.0, 999.0, 0.0], 0.0)}


def embed_case(S, Pz, Cn, D, B, generic, seed, ln=None):
    extras, normalize, t_vec, t_state = EMBED_MODES[B]
    x, w, bias, pos, label, y = embed_operands(B, Cn, S, Pz, D, extras, seed)
    t = np.asarray(t_vec if t_vec is not None else [t_state] * B, np.float64)
    want, tol = embed_ref(x, w, bias, pos, label, y, t, extras, normalize)
    xt, fr = run_embed(x, w, bias, pos, label, y, extras, normalize, generic, t_vec, t_state, ln)
    L = want.shape[1]
    Mp = xt.shape[0] - 8
    what = f"embed S={S} P={Pz} C={Cn} D={D} B={B} extras={extras} normalize={normalize} t={'per row' if t_vec is not None else 'StepState'} generic={generic}"
    assert np.all(xt[Mp:] == NAN32), what + ": the rows behind the workspace were written"
    assert not xt[B * L:Mp].any(), what + ": padding rows are not zero"
    got = xt[:B * L].view(np.float32).reshape(B, L, D)
    is_time = np.arange(L) == extras - 1
    r_time = gate(got[:, is_time], want[:, is_time], tol[:, is_time], what + " time token")
    r_rest = gate(got[:, ~is_time], want[:, ~is_time], tol[:, ~is_time], what + " patch and label tokens")
    print(f"{what}: error / bound {r_rest:.3f} (patch and label columns), {r_time:.3f} (time token)")
    return xt, fr, want, (x, w, bias, pos, label, y, extras, normalize, t_vec, t_state)


@gpu
@pytest.mark.parametrize("S,Pz,Cn,D", [(8, 2, 3, 64), (16, 2, 3, 128), (32, 4, 3, 192), (28, 4, 4, 256)])
def test_embed_generic_against_float64_reference(S, Pz, Cn, D):
    """embed_kernel on grids the MFMA kernel does not take (28 / 4 = 7 patches per row: neither 16 wide nor a power of two)"""
    for B in (1, 3, 2, 5):
        embed_case(S, Pz, Cn, D, B, generic=0, seed=S + B)


@gpu
@pytest.mark.parametrize("B", [1, 3, 9, 17])
@pytest.mark.parametrize("S,Pz,Cn,D", [(64, 4, 3, 512), (32, 2, 3, 512), (32, 2, 4, 768), (32, 2, 4, 1024), (64, 4, 3, 256)])
def test_embed_mfma_and_generic_against_float64_reference(S, Pz, Cn, D, B):
    """grids 16 patches wide: embed_mfma_kernel<4,3> / <2,3> / <2,4> (grid.y splits the column pairs at small B; a workgroup holds half an image),
    and embed_kernel on the same operands.  Whether the two are bit-equal is printed, not asserted."""
    mfma = embed_case(S, Pz, Cn, D, B, generic=0, seed=D + B)[0]
    gen = embed_case(S, Pz, Cn, D, B, generic=1, seed=D + B)[0]
    diff = int((mfma != gen).sum())
    print(f"embed S={S} P={Pz} C={Cn} D={D} B={B}: MFMA and generic kernels bit-equal: {diff == 0} ({diff} of {mfma.size} words differ)")


@gpu
@pytest.mark.parametrize("B", [1, 3, 9, 17])
def test_embed_with_norm1_in_fragment_order(B):
    """embed_mfma_kernel<4, 3, 512>: x_tok bit-equal to the plain launch's, the first block's norm1 of the patch rows in fragment order under the
    LayerNorm section's bf16 gate against the float64 LayerNorm of the float64 embedded rows"""
    r = np.random.default_rng(B)
    g = (1.0 + 0.2 * r.standard_normal(512)).astype(np.float32)
    b = (0.3 * r.standard_normal(512)).astype(np.float32)
    plain = embed_case(64, 4, 3, 512, B, generic=0, seed=40 + B)[0]
    xt, fr, want, ops = embed_case(64, 4, 3, 512, B, generic=0, seed=40 + B, ln=(g, b))
    assert np.array_equal(xt, plain), "x_tok differs from the launch without norm1"
    extras = ops[6]
    rows64 = want[:, extras:].reshape(B * 256, 512)
    ln_want = ln_ref(rows64, g, b)
    e32 = float(np.abs(ln_ref(rows64.astype(np.float32), g, b, np.float32).astype(np.float64) - ln_want).max())
    t16 = 2.0 ** -8 * np.abs(ln_want) + 2.0 * max(4.0 * e32, 2e-6)
    ratio = gate(from_bf16_bits(unfrag(fr, B * 8, 512)), ln_want, t16, f"embed + norm1 B={B}")
    print(f"embed + norm1 B={B}: error / bound {ratio:.3f}")
    assert np.all(fr.reshape(-1)[B * 256 * 512:] == NAN16), "the fragment buffer was written past its last group"


# ---------------------------------------------------------------------------------------------------------------- time_embed MLP
def time_mlp_ref(t, D, normalize, w1, b1, w2, b2, pos_row, dtype=np.float64, act="silu"):
    emb, _ = sinusoid(np.asarray(t, dtype), D, normalize, dtype)
    w1, b1, w2, b2, pos_row = (np.asarray(a, dtype) for a in (w1, b1, w2, b2, pos_row))
    h = emb @ w1.T + b1
    sig = dtype(1) / (dtype(1) + np.exp(-h))
    h = h * sig if act == "silu" else sig
    return h @ w2.T + b2 + pos_row


def time_mlp_operands(D, L, seed):
    r = np.random.default_rng(seed)
    w1 = (r.standard_normal((4 * D, D)) / np.sqrt(D)).astype(np.float32)
    b1 = (0.3 * r.standard_normal(4 * D)).astype(np.float32)
    w2 = (r.standard_normal((D, 4 * D)) / np.sqrt(4 * D)).astype(np.float32)
    b2 = (0.3 * r.standard_normal(D)).astype(np.float32)
    pos = (0.5 * r.standard_normal((L, D))).astype(np.float32)
    return w1, b1, w2, b2, pos


def time_mlp_tolerance(t, D, normalize, w1, b1, w2, b2, pos_row):
    want = time_mlp_ref(t, D, normalize, w1, b1, w2, b2, pos_row)
    e32 = float(np.abs(time_mlp_ref(t, D, normalize, w1, b1, w2, b2, pos_row, np.float32).astype(np.float64) - want).max())
    return want, max(8.0 * e32, 1e-6 * float(np.abs(want).max())), e32


@gpu
@pytest.mark.parametrize("D", [64, 256, 512])
def test_time_mlp_against_float64_reference(D):
    ctx = kernel_support.ctx()
    L = 9
    for B in (1, 5):
        for extras in (1, 2):
            for normalize in (0, 1):
                for source in ("per row", "StepState"):
                    w1, b1, w2, b2, pos = time_mlp_operands(D, L, seed=D + B + extras)
                    t_vec = np.asarray(([0.0, 999.0, 1.0, 999.0, 0.0] if source == "per row" else [999.0 if normalize else 0.0] * 5)[:B], np.float32)
                    if source == "per row" and B == 1:
                        t_vec[:] = 999.0
                    want, tol, e32 = time_mlp_tolerance(t_vec, D, normalize, w1, b1, w2, b2, pos[extras - 1])
                    x0 = np.random.default_rng(B).standard_normal((B, L, D)).astype(np.float32)
                    xt = x0.copy()
                    ctx.check(ctx.lib.dd_dev_time_mlp(ctx.handle, B, D, L, extras, normalize, P(w1), P(b1), P(w2), P(b2), P(pos),
                                                      P(t_vec) if source == "per row" else None, float(t_vec[0]), P(xt), 0, None,
                                                      C.byref(C.c_float(0))))
                    what = f"time_mlp D={D} B={B} extras={extras} normalize={normalize} t={t_vec.tolist()} ({source})"
                    ratio = gate(xt[:, extras - 1], want, tol, what)
                    others = np.arange(L) != extras - 1
                    assert np.array_equal(xt[:, others].view(np.uint32), x0[:, others].view(np.uint32)), what + ": another row changed"
                    print(f"{what}: error / bound {ratio:.3f} (e32 {e32:.2e}, max |err| {np.abs(xt[:, extras - 1] - want).max():.2e})")


# ---------------------------------------------------------------------------------------------------------------- the gates themselves (CPU)
def test_gates_reject_the_bugs_they_are_meant_to_catch():
    """The gates above reject: a fragment-order store with the two lane halves exchanged; an extra token (label, time) that takes the pos_embed
    row behind its own; SiLU replaced by a plain sigmoid.  What a correct kernel returns -- the reference rounded to the output type, or
    evaluated in float32 -- passes."""
    # LayerNorm in fragment order
    D, tok_l, tok_e, nimg = 256, 33, 1, 3
    x, g, b = ln_rows(nimg * tok_l, D, 100.0, 1.0, 1)
    want, t32, t16 = ln_tolerances(x, g, b)
    patch = want[(np.arange(nimg * tok_l) % tok_l) >= tok_e]
    t16p = t16[(np.arange(nimg * tok_l) % tok_l) >= tok_e]
    good = bf16(patch.astype(np.float32))
    assert gate(want.astype(np.float32), want, t32, "fp32 of the reference") < 1.0
    assert gate(ln_ref(x, g, b, np.float32), want, t32, "float32 evaluation") <= 0.25 + 1e-12
    assert gate(unfrag(to_frag(good, D), nimg, D), patch, t16p, "bf16 of the reference through the fragment order") < 1.0
    with pytest.raises(AssertionError):
        gate(unfrag(to_frag(good, D, swap_halves=True), nimg, D), patch, t16p, "lane halves exchanged")
    # token assembly
    for extras in (1, 2):
        B = 3
        x, w, bias, pos, label, y = embed_operands(B, 3, 16, 2, 128, extras, 2)
        t = np.asarray([0.0, 1.0, 999.0])
        want, tol = embed_ref(x, w, bias, pos, label, y, t, extras, 0)
        f32 = (x.reshape(B, 3, 8, 2, 8, 2).transpose(0, 2, 4, 1, 3, 5).reshape(B, 64, 12) @ w.reshape(128, 12).T + bias + pos[extras:]).astype(np.float32)
        assert gate(f32, want[:, extras:], tol[:, extras:], "float32 evaluation of the patch tokens") < 1.0
        assert gate(want.astype(np.float32), want, tol, "fp32 of the reference") < 1.0
        bad, _ = embed_ref(x, w, bias, pos, label, y, t, extras, 0, pos_shift=1)
        for row in range(extras):
            with pytest.raises(AssertionError):
                gate(bad[:, row], want[:, row], tol[:, row], f"extras={extras}: token {row} with the next pos_embed row")
    # time_embed MLP
    for D, normalize in ((64, 0), (256, 1)):
        w1, b1, w2, b2, pos = time_mlp_operands(D, 4, 3)
        t = np.asarray([0.0, 999.0, 1.0], np.float32)
        want, tol, _ = time_mlp_tolerance(t, D, normalize, w1, b1, w2, b2, pos[0])
        assert gate(time_mlp_ref(t, D, normalize, w1, b1, w2, b2, pos[0], np.float32), want, tol, "float32 evaluation") <= 0.125 + 1e-12
        with pytest.raises(AssertionError):
            gate(time_mlp_ref(t, D, normalize, w1, b1, w2, b2, pos[0], act="sigmoid"), want, tol, "SiLU replaced by sigmoid")
