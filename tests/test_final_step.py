"""GPU unit tests of the launch that ends every sampling step and every forward (csrc/step.hip final_tiled_kernel: unpatchify, the 3x3 conv,
guidance, the step update, the known region, the Philox draw) through its development entry point dd_dev_final (include/duodiff_dev.h).

What is compared with what (the references and their CPU tests: tests/kernel_support.py, tests/test_kernel_support.py):
  eps_out   per element against the float64 head final_eps64, within its derived bound (an fmaf chain of 9 C terms on the bias; guided: the
            two convs' bounds through c + s (c - u) and that expression's three roundings) -- no fitted number;
  x_out, h, the twin image   bit for bit against the float32 restatement of step_update.h applied to the kernel's OWN eps_out of the same
            launch: the conv is judged above, the update has no tolerance;
  what must not be written   every canary, the image past the last one of every buffer, buffers the launch is not handed, h without history;
  the step state   t, t_model, t_final, seed after the launch;
  the device noise   per element against philox_normal4_ref (integer Philox4x32-10, float32 uniforms, float64 sqrt / log / sin / cos).

Inputs: standard-normal decoder rows and conv weights (neither symmetric nor separable), NaN in the decoder rows of the extra tokens of dec and
dec2 (never read), B = 3 images so that a wrong batch stride cannot hide.

Instantiations (4 (C, P) forms x G x H x K = 32) and tile geometries reached:
  test_every_instantiation_at_two_by_two_tiles   S = 32 (2 x 2 full tiles): each of the compiled forms <3,4>, <3,2>, <4,2> and the run-time form
            <0,0> at (1,1), (2,2), (3,1), (4,4), (1,8) runs {plain, classifier-free, autoguided} x {history off / on} x {known region off / on}:
            all 32 instantiations, G = true from both of its callers.  History off: the DDPM rule; on: a table row.
  test_every_tile_geometry   the same eight (C, P) at S = 8 (one partial tile, 64 live lanes), 16 (exactly one tile), 24 (2 x 2 tiles, the last
            row and column with 8 live lanes), 48 (3 x 3: one tile has neighbours on all four sides): the plain forward-only launch
            <CT,PT,0,0,0> and the fullest ones <CT,PT,1,1,1>, classifier-free and autoguided (extras2 != extras, a conv of its own).
  test_one_64_pixel_image   S = 64 (4 x 4 tiles), B = 1, <3,4,0,0,0> and <3,4,1,1,1>.
  test_batched_early_exit_heads   layer_B: 3 layers of 2 images, each layer its own conv through w_stride / b_stride, <CT,PT,0,0,0> forward-only.
  test_step_rules_bit_for_bit   <3,4,*,*,*> and <0,0,*,*,*> at S = 24: DDPM at t = 0 / 1 / 999 with both variances, table rows with and without
            noise, history with hist = 0 on a NaN h and hist = 1, the known region with kb = 0 and kb != 0, advance set and clear.
  test_philox_*   <3,*>, <4,2> and <0,0> (C = 1) with K off (z) and on (z2), S = 24 / 32 / 64.
"""
import ctypes as C

import numpy as np
import pytest

import kernel_support as ks
from duodiff_amd import _lib
from kernel_support import F32, P, untouched

pytestmark = pytest.mark.gpu

DDPM = dict(c1=1.0123, c2=0.0871, sigma_tilde=0.31, sigma_beta=0.42)
ROW = dict(t_model=417.25, a=0.9731, b=-0.2173, c=0.3337, noise=1, ctr=11, next_t_model=391.5)
HIST = dict(d=0.1291, p=1.0413, q=-0.3127, hist=1)
KNOWN = dict(ka=0.8125, kb=0.5829)


class Out:
    pass


def launch(a, *, write_eps=True, write_x=False, x_alias=True, x_in=None, z=None, h=None, kx0=None, kmask=None, t=0, seed=0, advance=0,
           noise_mode=_lib.DD_NOISE_NONE, variance=0, ddpm=None, row=None, hist=None, known=None, b0=0, expect=_lib.DD_OK, **override):
    """one dd_dev_final call on the operands `a` (kernel_support.final_inputs); returns the whole buffers and the step state read back.
    override: fields of dd_dev_final_args set last, by name (the rejected calls)"""
    ctx = ks.ctx()
    B, Cn, S = a["B"], a["C"], a["S"]
    img = Cn * S * S
    images = (2 * B if a.get("pair_B") else B) + 1
    q = _lib.dd_dev_final_args()
    keep = []

    def ptr(arr):
        if arr is None:
            return None
        arr = np.ascontiguousarray(arr, F32)
        keep.append(arr)
        return arr.ctypes.data

    q.B, q.C, q.S, q.P, q.L, q.extras, q.b0, q.images = B, Cn, S, a["P"], a["L"], a["extras"], b0, images
    q.dec, q.wconv, q.bconv = ptr(a["dec"]), ptr(a["wconv"]), ptr(a["bconv"])
    q.dec2, q.wconv2, q.bconv2 = ptr(a.get("dec2")), ptr(a.get("wconv2")), ptr(a.get("bconv2"))
    q.L2, q.extras2, q.pair_B, q.layer_B = a.get("L2", 0), a.get("extras2", 0), a.get("pair_B", 0), a.get("layer_B", 0)
    q.w_stride, q.b_stride, q.guide_scale = a.get("w_stride", 0), a.get("b_stride", 0), a.get("scale", 0.0)
    q.write_eps, q.write_x, q.x_alias = int(write_eps), int(write_x), int(x_alias)
    o = Out()
    o.eps, o.x = np.zeros(images * img + 8, F32), np.zeros(images * img + 8, F32)
    o.h = None if h is None else np.ascontiguousarray(h, F32).copy()
    q.eps_out, q.x_out, q.x_in, q.z, q.h = P(o.eps), P(o.x), ptr(x_in), ptr(z), P(o.h)
    q.t, q.advance, q.noise_mode, q.variance, q.seed = t, advance, noise_mode, variance, seed
    if row is not None:
        q.table = 1
        q.row_t_model, q.row_a, q.row_b, q.row_c, q.row_noise, q.row_ctr, q.next_t_model = (row[k] for k in ("t_model", "a", "b", "c", "noise", "ctr", "next_t_model"))
    if ddpm is not None:
        q.c1, q.c2, q.sigma_tilde, q.sigma_beta = (ddpm[k] for k in ("c1", "c2", "sigma_tilde", "sigma_beta"))
    if hist is not None:
        q.hist_row, q.hist_d, q.hist_p, q.hist_q, q.hist = 1, hist["d"], hist["p"], hist["q"], hist["hist"]
    if known is not None:
        q.known, q.known_ka, q.known_kb = 1, known["ka"], known["kb"]
    q.kx0, q.kmask = ptr(kx0), ptr(kmask)
    q.t_out = q.t_final_out = -12345
    for k, v in override.items():
        setattr(q, k, v)
    rc = ctx.lib.dd_dev_final(ctx.handle, C.byref(q), None)
    assert rc == expect, (rc, ctx.lib.dd_last_error(ctx.handle))
    o.q, o.images, o.img = q, images, img
    return o


def ff(*shape):
    """float32 of 0xFF bytes"""
    v = np.empty(shape, F32)
    v.view(np.uint32)[...] = ks.NAN32
    return v


def step_operands(a, seed, nan_h=False):
    """x, z, h, the known image and a mask of 0, 1 and fractions; 0xFF bytes in the images of x and h past the launch's own (and in h's canary);
    NaN in the known image wherever the mask is 0"""
    r = np.random.default_rng(seed)
    B, Cn, S = a["B"], a["C"], a["S"]
    images = (2 * B if a.get("pair_B") else B) + 1
    x, h = ff(images, Cn, S, S), ff(images * Cn * S * S + 8)
    x[:B] = r.standard_normal((B, Cn, S, S))
    if not nan_h:
        h[:B * Cn * S * S] = r.standard_normal(B * Cn * S * S)
    z = r.standard_normal((B, Cn, S, S)).astype(F32)
    kmask = r.choice(np.array([0.0, 0.0, 1.0, 1.0, 0.25, 0.7], F32), (B, 1, S, S))
    kx0 = np.where(kmask == 0, F32(np.nan), r.standard_normal((B, Cn, S, S)).astype(F32)).astype(F32)
    return x, z, h, kx0, kmask


def check_eps(a, o, what):
    """eps_out of the launch's B images within the derived bound; the image past them and the canary untouched.  Returns error / bound"""
    B, n = a["B"], a["B"] * o.img
    want, tol = ks.final_eps64(**a)
    ratio = ks.gate(o.eps[:n].reshape(want.shape), want, tol, what)
    assert untouched(o.eps[n:]), f"{what}: eps_out written past image {B}"
    return ratio


def run_step(a, what, *, t=5, variance=0, noise_mode=_lib.DD_NOISE_BUFFER, table=False, noise=1, hist=None, known=None, advance=1,
             x_alias=True, nan_z=False, seed=0x9E3779B97F4A7C15):
    """one whole step: launch, then every check the module docstring lists.  Returns (error / bound of eps, the launch's outputs)"""
    B, Cn, S, n = a["B"], a["C"], a["S"], a["B"] * a["C"] * a["S"] * a["S"]
    x, z, h, kx0, kmask = step_operands(a, 31 * S + Cn, nan_h=hist is not None and not hist["hist"])
    if nan_z:
        z[:] = np.nan
    row = dict(ROW, noise=noise) if table else None
    o = launch(a, write_x=True, x_alias=x_alias, x_in=x, z=z, h=h, kx0=kx0 if known else None, kmask=kmask if known else None, t=t, seed=seed,
               advance=advance, noise_mode=noise_mode, variance=variance, ddpm=None if table else DDPM, row=row, hist=hist, known=known)
    ratio = check_eps(a, o, what)
    eps = o.eps[:n].reshape(B, Cn, S, S)
    # ---- x', h' from the kernel's own eps, in float32
    if table:
        zz = z if row["noise"] and noise_mode == _lib.DD_NOISE_BUFFER else None
        hh = h[:n].reshape(x[:B].shape)
        d, use = (hist["d"], hist["hist"]) if hist else (0.0, 0)
        xp = ks.step_table(x[:B], eps, zz, hh, row["a"], row["b"], row["c"], d, use)
    else:
        zz = z if t > 0 and noise_mode == _lib.DD_NOISE_BUFFER else None
        xp = ks.step_ddpm(x[:B], eps, zz, DDPM["c1"], DDPM["c2"], DDPM["sigma_beta" if variance == 1 else "sigma_tilde"])
    if known:
        xp = ks.step_known(xp, kx0, np.broadcast_to(kmask, xp.shape), known["ka"], known["kb"], None)      # (no z2 outside the Philox mode)
    assert np.isfinite(xp).all(), f"{what}: the restated x' is not finite"
    got = o.x[:n].reshape(xp.shape)
    assert np.array_equal(got.view(np.uint32), xp.view(np.uint32)), f"{what}: x' differs from the restatement in {(got != xp).sum()} of {n} elements"
    twin = a.get("pair_B", 0) > 0
    if twin:
        assert np.array_equal(o.x[n:2 * n].view(np.uint32), o.x[:n].view(np.uint32)), f"{what}: the twin image differs from image b"
    assert untouched(o.x[(2 * n if twin else n):]), f"{what}: x_out written past its images (autoguided: no twin is written)"
    if hist:
        hp = ks.step_history(x[:B], eps, hist["p"], hist["q"])
        assert np.isfinite(hp).all() and np.array_equal(o.h[:n].view(np.uint32), hp.reshape(-1).view(np.uint32)), f"{what}: h' differs"
        assert untouched(o.h[n:]), f"{what}: h written past image {B}"
    else:
        assert np.array_equal(o.h.view(np.uint32), h.view(np.uint32)), f"{what}: h written without history"
    # ---- the step state
    t0_model = row["t_model"] if table else float(t)
    want_state = ((t + 1, row["next_t_model"]) if table else (t - 1, float(t - 1))) if advance else (t, t0_model)
    assert (o.q.t_out, o.q.t_model_out, o.q.t_final_out, o.q.seed_out) == (want_state[0], want_state[1], t, seed), what
    return ratio, o


def combo(guided, hist, known):
    return dict(table=hist, hist=dict(HIST) if hist else None, known=dict(KNOWN, kb=0.0 if guided == "auto" else KNOWN["kb"]) if known else None)


RATIOS = {}


def note(C_, P_, ratio):
    form = (C_, P_) if (C_, P_) in ks.FINAL_FORMS[:3] else (0, 0)
    RATIOS[form] = max(RATIOS.get(form, 0.0), ratio)
    print(f"eps error / bound {ratio:.3f}; largest so far for form <{form[0]},{form[1]}>: {RATIOS[form]:.3f}")


@pytest.mark.parametrize("known", [False, True], ids=["", "known"])
@pytest.mark.parametrize("hist", [False, True], ids=["", "hist"])
@pytest.mark.parametrize("guided", [None, "cfg", "auto"], ids=["plain", "cfg", "auto"])
@pytest.mark.parametrize("C_,P_", ks.FINAL_FORMS)
def test_every_instantiation_at_two_by_two_tiles(C_, P_, guided, hist, known):
    a = ks.final_head_inputs(C_, P_, 32, guided)
    ratio, _ = run_step(a, f"C{C_} P{P_} S32 {guided} hist={hist} known={known}", **combo(guided, hist, known))
    note(C_, P_, ratio)


@pytest.mark.parametrize("S", [8, 16, 24, 48])
@pytest.mark.parametrize("C_,P_", ks.FINAL_FORMS)
def test_every_tile_geometry(C_, P_, S):
    a = ks.final_head_inputs(C_, P_, S)
    o = launch(a)                                             # the forward-only launch: eps_out alone
    note(C_, P_, check_eps(a, o, f"C{C_} P{P_} S{S} forward"))
    assert untouched(o.x), "the x_out of a forward-only launch"
    assert (o.q.t_out, o.q.t_final_out) == (0, 0)
    for guided in ("cfg", "auto"):
        a = ks.final_head_inputs(C_, P_, S, guided)
        assert guided != "auto" or a["extras2"] != a["extras"]
        ratio, _ = run_step(a, f"C{C_} P{P_} S{S} {guided} fullest", x_alias=guided == "cfg", **combo(guided, True, True))
        note(C_, P_, ratio)


def test_one_64_pixel_image():
    a = ks.final_head_inputs(3, 4, 64, B=1)
    note(3, 4, run_step(a, "S64 plain")[0])
    a = ks.final_head_inputs(3, 4, 64, "cfg", B=1)
    note(3, 4, run_step(a, "S64 fullest", **combo("cfg", True, True))[0])


@pytest.mark.parametrize("C_,P_,S", [(3, 4, 32), (3, 4, 24), (2, 2, 24), (4, 2, 32)])
def test_batched_early_exit_heads(C_, P_, S):
    """3 layers of 2 images: layer i convolves with wconv + i w_stride / bconv + i b_stride (the gaps between the layers' weights hold NaN)"""
    a = ks.final_inputs(C_, P_, S, 6, 1, 77 + S + C_, layers=3)
    assert a["layer_B"] == 2 and a["w_stride"] > 9 * C_ * C_
    o = launch(a)
    note(C_, P_, check_eps(a, o, f"heads C{C_} P{P_} S{S}"))
    assert untouched(o.x)


STEPS = {
    "ddpm_t0_nan_z": dict(t=0, nan_z=True),                                   # no noise at t = 0: the z buffer must not matter
    "ddpm_t0_beta": dict(t=0, variance=1, nan_z=True, advance=0),
    "ddpm_t1_tilde": dict(t=1, variance=0),
    "ddpm_t1_beta": dict(t=1, variance=1),
    "ddpm_t999_tilde": dict(t=999, variance=0, advance=0),
    "ddpm_t999_beta": dict(t=999, variance=1),
    "ddpm_no_noise_mode": dict(t=7, noise_mode=_lib.DD_NOISE_NONE, nan_z=True),
    "ddpm_known_kb": dict(t=3, known=dict(KNOWN)),
    "table_noise": dict(t=4, table=True, noise=1),
    "table_no_noise": dict(t=0, table=True, noise=0, nan_z=True),
    "table_hist0_nan_h": dict(t=0, table=True, hist=dict(HIST, hist=0)),       # x' finite, h' written
    "table_hist1": dict(t=9, table=True, hist=dict(HIST), advance=0),
    "table_hist1_known_kb0": dict(t=2, table=True, noise=0, hist=dict(HIST), known=dict(KNOWN, kb=0.0)),
    "table_known_kb": dict(t=300, table=True, known=dict(KNOWN)),
}


@pytest.mark.parametrize("name", list(STEPS))
@pytest.mark.parametrize("C_,P_,guided", [(3, 4, None), (3, 4, "cfg"), (2, 2, "auto")])
def test_step_rules_bit_for_bit(C_, P_, guided, name):
    a = ks.final_head_inputs(C_, P_, 24, guided)
    step = STEPS[name]
    ratio, o = run_step(a, f"{name} C{C_} {guided}", **step)
    note(C_, P_, ratio)
    _, o2 = run_step(a, f"{name} C{C_} {guided}, x_out apart from x_in", x_alias=False, **step)      # x_out aliasing x_in against a separate output
    for k in ("eps", "x", "h"):
        assert np.array_equal(getattr(o, k).view(np.uint32), getattr(o2, k).view(np.uint32)), k


def test_buffers_the_launch_is_not_handed_stay_untouched():
    a = ks.final_head_inputs(3, 4, 24)
    x, z, h, _, _ = step_operands(a, 5)
    o = launch(a, write_eps=False, write_x=True, x_in=x, z=z, h=h, t=3, noise_mode=_lib.DD_NOISE_BUFFER, ddpm=DDPM)      # eps_out unset
    assert untouched(o.eps) and not untouched(o.x[:a["B"] * o.img]) and np.array_equal(o.h.view(np.uint32), h.view(np.uint32))
    o2 = launch(a, write_eps=True, write_x=True, x_in=x, z=z, h=h, t=3, noise_mode=_lib.DD_NOISE_BUFFER, ddpm=DDPM)
    assert np.array_equal(o.x.view(np.uint32), o2.x.view(np.uint32)), "x' must not depend on whether eps is written"
    o3 = launch(a, write_eps=True, write_x=False, x_in=x, z=z, t=3, advance=1, ddpm=DDPM)                                   # x_out unset: only the state moves
    assert untouched(o3.x) and np.array_equal(o3.eps.view(np.uint32), o2.eps.view(np.uint32)) and (o3.q.t_out, o3.q.t_final_out) == (2, 3)


def test_rejected_calls_come_back_as_error_codes():
    """every check of the entry point: DD_ERR_INVALID, nothing launched, no buffer written"""
    a = ks.final_head_inputs(3, 4, 16)
    x, z, h, kx0, kmask = step_operands(a, 1)
    ok = dict(write_x=True, x_in=x, z=z, t=3, noise_mode=_lib.DD_NOISE_BUFFER, ddpm=DDPM)
    tab = dict(ok, row=ROW, ddpm=None, h=h)
    g = ks.final_head_inputs(3, 4, 16, "auto")
    bad = [(a, ok, over) for over in (
        dict(C=0), dict(C=5), dict(P=5), dict(P=0), dict(S=18), dict(S=2048), dict(B=4097, images=4098), dict(L=a["L"] + 1), dict(extras=a["extras"] + 1), dict(extras=-1), dict(B=0),
        dict(images=2), dict(b0=-1), dict(t=1000), dict(t=-1), dict(noise_mode=3), dict(variance=2), dict(dec=None), dict(wconv=None),
        dict(bconv=None), dict(x_in=None), dict(x_out=None), dict(z=None), dict(eps_out=None), dict(pair_B=2), dict(pair_B=3), dict(layer_B=2),
        dict(layer_B=3, pair_B=3, images=7), dict(hist=HIST, h=h), dict(known=KNOWN), dict(dec2=a["dec"].ctypes.data))]
    bad += [(a, tab, over) for over in (dict(t=65536), dict(t=-1), dict(hist=HIST, h=None), dict(hist=HIST, write_x=False), dict(known=KNOWN, kx0=kx0),
                                        dict(known=KNOWN, kmask=kmask), dict(known=KNOWN, kx0=kx0, kmask=kmask, write_x=False),
                                        dict(layer_B=3, hist=HIST), dict(layer_B=3, known=KNOWN, kx0=kx0, kmask=kmask))]
    bad += [(g, ok, over) for over in (dict(wconv2=None), dict(bconv2=None), dict(L2=g["L2"] + 1), dict(extras2=-1), dict(pair_B=3, images=7), dict(layer_B=3))]
    for ops, base, over in bad:
        o = launch(ops, expect=_lib.DD_ERR_INVALID, **{**base, **over})
        assert np.all(o.eps == 0) and np.all(o.x == 0) and o.q.t_out == -12345, over
    assert ks.ctx().lib.dd_dev_final(ks.ctx().handle, None, None) == _lib.DD_ERR_INVALID
    launch(a, **ok)                                           # the calls above with nothing overridden are accepted
    launch(a, **dict(tab, hist=HIST, known=KNOWN, kx0=kx0, kmask=kmask))
    launch(g, **ok)


# ---------------------------------------------------------------------------------------------------------------- the device noise
# |z - ref| of the kernel's draw against philox_normal4_ref is the error of the hardware log, sin and cos (and three fp32 roundings); it cannot be
# derived from anything in the project.  Measured on an MI355X over PHILOX_CASES (56 832 draws, max |z| 4.24): 1.353e-6 at the worst case,
# 1.08e-6 .. 1.35e-6 over the seven; the bound is 4 x that, 5.412e-6 (draws not in the sample; the error grows towards |z| ~ 6.7), far below the
# 1e-4 it may not exceed -- a mix-up of id, counter, stream or seed is an error of order 1.  The draws whose uniform rounds to within 2^-10 of 1
# (log near 0) measured 1.3e-8 at most: they need no bound of their own and are held to the same one.
PHILOX_MEASURED = 1.353e-6
PHILOX_BOUND = 4 * PHILOX_MEASURED
assert PHILOX_BOUND <= 1e-4


def draw(case, b0=None, ddpm=False):
    """z (row (0, 0, 1) on finite inputs: 0 + 0 + 1 z) or z2 (row (0, 0, 0), ka = 0, kb = 1, x0 = 0, m = 1) of a case, as the launch returns it"""
    a = ks.final_inputs(case["C"], 2 if case["S"] < 64 else 4, case["S"], case["B"], 1, 5)
    B, Cn, S = case["B"], case["C"], case["S"]
    x = ff(B + 1, Cn, S, S)
    x[:B] = np.random.default_rng(2).standard_normal((B, Cn, S, S))
    kw = dict(write_x=True, x_in=x, seed=case["seed"], noise_mode=_lib.DD_NOISE_PHILOX, b0=case["b0"] if b0 is None else b0)
    if case["z2"]:
        o = launch(a, row=dict(ROW, a=0.0, b=0.0, c=0.0, noise=0, ctr=case["ctr"]), t=6, known=dict(ka=0.0, kb=1.0),
                   kx0=np.zeros((B, Cn, S, S), F32), kmask=np.ones((B, 1, S, S), F32), **kw)
    elif ddpm:
        o = launch(a, t=case["ctr"], ddpm=dict(c1=0.0, c2=1.0, sigma_tilde=1.0, sigma_beta=np.nan), **kw)
    else:
        o = launch(a, row=dict(ROW, a=0.0, b=0.0, c=1.0, noise=1, ctr=case["ctr"]), t=6, **kw)
    n = B * Cn * S * S
    assert untouched(o.x[n:])
    return o.x[:n].reshape(B, Cn, S, S).astype(np.float64)


@pytest.mark.parametrize("case", ks.PHILOX_CASES, ids=lambda c: f"S{c['S']}-C{c['C']}-b{c['b0']}-k{c['ctr']}-{'z2' if c['z2'] else 'z'}")
def test_philox_draw_against_the_host_reference(case):
    stream = ks.PHILOX_KNOWN if case["z2"] else ks.PHILOX_STEP
    want, near = ks.final_philox_ref(case["seed"], case["B"], case["C"], case["S"], case["b0"], case["ctr"], stream)
    got = draw(case)
    err = np.abs(got - want)
    print(f"philox: max |z - ref| {err.max():.3e} (draws with the uniform within 2^-10 of 1: {err[near].max() if near.any() else 0.0:.3e}, "
          f"{near.mean():.4f} of the case); max |z| {np.abs(want).max():.2f}")
    ks.gate(got, want, PHILOX_BOUND, "philox z against philox_normal4_ref")
    if case["b0"] == 5:        # image b of the launch that starts at image 5 is image b + 5 of the undivided batch
        whole, _ = ks.final_philox_ref(case["seed"], case["B"] + 5, case["C"], case["S"], 0, case["ctr"], stream)
        ks.gate(got, whole[5:], PHILOX_BOUND, "b0 = 5 against images 5.. of a b0 = 0 reference")


def test_philox_ddpm_counter_is_the_timestep():
    case = dict(S=24, B=3, C=3, b0=0, seed=0x1234, ctr=941, z2=False)
    want, _ = ks.final_philox_ref(case["seed"], 3, 3, 24, 0, 941)
    ks.gate(draw(case, ddpm=True), want, PHILOX_BOUND, "the DDPM rule's z: counter word = t")


def test_philox_step_is_the_composition_of_its_draws():
    """a whole table step with history and a known region in the Philox mode, bit for bit from the kernel's own eps and its own z and z2"""
    case = dict(S=24, B=3, C=3, b0=5, seed=(7 << 32) | 0x9ABCDEF1, ctr=ROW["ctr"], z2=False)
    z, z2 = draw(case).astype(F32), draw(dict(case, z2=True)).astype(F32)
    a = ks.final_head_inputs(3, 2, 24, "cfg")
    x, _, h, kx0, kmask = step_operands(a, 9)
    o = launch(a, write_x=True, x_in=x, h=h, kx0=kx0, kmask=kmask, t=6, seed=case["seed"], noise_mode=_lib.DD_NOISE_PHILOX, row=ROW, hist=HIST,
               known=KNOWN, b0=5)
    check_eps(a, o, "philox step")
    n = 3 * o.img
    eps = o.eps[:n].reshape(z.shape)
    xp = ks.step_table(x[:3], eps, z, h[:n].reshape(z.shape), ROW["a"], ROW["b"], ROW["c"], HIST["d"], 1)
    xp = ks.step_known(xp, kx0, np.broadcast_to(kmask, xp.shape), KNOWN["ka"], KNOWN["kb"], z2)
    assert np.array_equal(o.x[:n].view(np.uint32), xp.reshape(-1).view(np.uint32))
    assert np.array_equal(o.x[n:2 * n].view(np.uint32), o.x[:n].view(np.uint32)) and untouched(o.x[2 * n:])
