"""Resampling jumps in the device loops (GPU): dd_jump_step, dd_sample_affine_walk (engine.sample_affine_walk_loop) and get_samples'
resample_jump / resample_count / restart.

The rule against a numpy fp32 restatement; the device walk against forward + affine_step + known_blend + jump_step with z, z2 and z3 as the
loop draws them (DDIM and predict_noise DDPM as affine rows; a region, both kinds of guidance, per-image seeds); graph == eager, two chains
== one, cut == uncut; a walk without jumps == dd_sample_affine; a jump that crosses the switch upward; the independence of z3; replay and
stale bytes; the rejected calls; the fp32 engine against the numpy oracle; the product width; the command line.  Bit for bit unless a bound
is named.
"""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, TINY
from duodiff_amd import _lib as L
from duodiff_amd.config import ModelParams, load_config
from duodiff_amd.weights import synthetic_state_dict
from loop_support import NULL, dev_flags, known_region, labels, philox_z, philox_z2, philox_z3, region_inputs, run_loop, run_steps, side_stream
from loop_support import tiny_model, uvit

pytestmark = pytest.mark.gpu
CELEBA_3 = REPO / "configs" / "uvit_celeba_3.yaml"


def _plan(kind, **kw):
    """the (6, 2, 2) walk -- S0 S1 S2 J(3->1) S1 S2 S3 S4 J(5->3) S3 S4 S5, 12 rows, jumps at rows 3 and 8 -- over 6 DDIM steps (eta 0.01)
    or over the 6 predict_noise DDPM steps from t = 5 as affine rows; both end on the final image"""
    from duodiff_amd import step_plan as sp
    kw = dict(dict(resample_jump=2, resample_count=2), **kw)
    if kind == "ddim":
        p = sp.step_plan(None, use_ddim=True, ddim_steps=7, ddim_eta=0.01, **kw)
    else:
        p = sp.step_plan("predict_noise", strength=5 / 999, **kw)
    assert p.kind == "affine" and p.rows["jump"].tolist() == [0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0] and p.lands[-1] == -1
    return p


def _walk(plan, first, x_in, stream, *, rows=None, region=None, **kw):
    """the device walk of the plan's rows (rows: others, e.g. without a late row; the region's (ka, kb) are the plan's); kw: run_loop's
    -> (x, chains of the last call)"""
    region = None if region is None else known_region(plan, *region)
    x, _, chains = run_loop("walk", first, x_in, plan.rows if rows is None else rows, stream, region=region, **kw)
    return x, chains


def _step_by_step(plan, first, x_in, stream, **kw):
    """row by row: a step is forward[_guided | _autoguided] of the row's model + affine_step [+ known_blend], a jump is jump_step, with z,
    z2 and z3 as the device loop draws them at the row's counter"""
    return run_steps("walk", first, x_in, plan, stream, **kw)[0]


# ---- 1. the rule ----------------------------------------------------------------------------------------------------------------
def _jump_numpy(x, z, ja, jc):
    """the rule, op by op in float32"""
    x, ja, jc = np.asarray(x, np.float32), np.float32(ja), np.float32(jc)
    v = ja * x
    if z is not None:
        v = v + jc * np.asarray(z, np.float32)
    assert v.dtype == np.float32
    return v


@pytest.mark.parametrize("shape", [(2, 3, 8, 8), (3, 4, 5, 5), (1, 1, 19, 19)])
def test_jump_step_kernel_bit_exact(shape):
    """dd_jump_step == the numpy restatement: 384 elements (whole 16-byte groups), 300 (a ragged last block) and 361 (a partial last
    group, finished element by element); with and without z; aliased and not; and from a pointer that is not 16-byte aligned (the
    scalar form)."""
    from duodiff_amd.engine import Context
    ctx = Context.get()
    g = torch.Generator().manual_seed(17)
    x, z = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    n = x.numel()
    for ja, jc in ((0.8431, 0.5377), (1.0, 0.0), (0.0, 1.0), (0.10636576, 0.99432707)):
        for with_z in (True, False):
            want = _jump_numpy(x.numpy(), z.numpy() if with_z else None, ja, jc)
            xd, zd = x.cuda(), z.cuda() if with_z else None
            out = ctx.jump_step(xd, zd, ja, jc)
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), want), (ja, jc, with_z)
            assert torch.equal(xd.cpu(), x), "the input was written"
            ctx.jump_step(xd, zd, ja, jc, out=xd)                                  # in place
            torch.cuda.synchronize()
            assert np.array_equal(xd.cpu().numpy(), want), (ja, jc, with_z, "aliased")
    xo, zo, oo = (torch.zeros(n + 1, device="cuda")[1:] for _ in range(3))         # 4 bytes past a 16-byte boundary
    assert xo.data_ptr() % 16 == 4 and xo.is_contiguous()
    xo.copy_(x.flatten()), zo.copy_(z.flatten())
    ctx.jump_step(xo, zo, 0.8431, 0.5377, out=oo)
    torch.cuda.synchronize()
    assert np.array_equal(oo.cpu().numpy().reshape(shape), _jump_numpy(x.numpy(), z.numpy(), 0.8431, 0.5377))
    with pytest.raises(ValueError, match="null tensor"):
        ctx.check(ctx.lib.dd_jump_step(ctx.handle, None, None, 1.0, 0.0, None, 4, None))


# ---- 2. the loop against the steps ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "region", "guided", "guided_region", "autoguided", "autoguided_region", "seeds", "seeds_region"])
@pytest.mark.parametrize("kind", ["ddim", "ddpm"])
def test_walk_equals_the_steps(kind, variant):
    """The device walk == forward + affine_step + known_blend + jump_step, row by row.  Guided, the steps behind a jump read the twin
    rows the jump wrote: a jump that left them behind would show in every later step.  B = 6 with the chain split forced but for the plain
    cases (B = 2, one chain)."""
    from duodiff_amd.engine import Autoguidance
    what, _, reg = variant.partition("_")
    B = 2 if what == "plain" or variant == "region" else 6
    guidance = y = seeds = None
    if what == "guided":
        m = tiny_model(2 * B, num_classes=11)
        y = labels(B, NULL, 6)
        guidance = (0.4, NULL)
    elif what == "autoguided":
        m = tiny_model(B)
        guidance = Autoguidance(tiny_model(B, seed=41, depth=1), 0.7)
    else:
        m = tiny_model(B)
        seeds = [11, 2 ** 63 + 5, 11, 3, 2 ** 64 - 1, 0][:B] if what == "seeds" else None
    x, x0, mask = region_inputs(B, 33)
    region = (x0, mask) if reg or variant == "region" else None
    plan, st = _plan(kind), side_stream()
    flags = L.DD_DEV_FORCE_CHAINS if B == 6 else 0
    xw, chains = _walk(plan, m, x, st, region=region, guidance=guidance, y=y, flags=flags, image_seeds=seeds)
    xs = _step_by_step(plan, m, x, st, region=region, guidance=guidance, y=y, image_seeds=seeds)
    assert chains == (2 if B == 6 else 1) and torch.isfinite(xw).all()
    assert torch.equal(xw, xs), "the device walk differs from the steps and jumps taken one by one"
    if region is not None:
        keep = (mask == 1).expand_as(x0)
        assert torch.equal(xw[keep], x0[keep]), "the known pixels of the result are not the known image"
    if seeds is not None:
        xu, _ = _walk(plan, m, x, st, region=region, flags=flags)
        assert not torch.equal(xw, xu), "the image seeds changed nothing"


# ---- 3. loop forms ----------------------------------------------------------------------------------------------------------------
def test_graph_equals_eager_and_two_chains_equal_one():
    B = 6
    m = tiny_model(B)
    x, x0, mask = region_inputs(B, 34)
    plan, st = _plan("ddim"), side_stream()
    xg, c1 = _walk(plan, m, x, st, region=(x0, mask), flags=L.DD_DEV_NO_CHAINS)
    xe, _ = _walk(plan, m, x, st, region=(x0, mask), use_graph=False)
    x2, c2 = _walk(plan, m, x, st, region=(x0, mask), flags=L.DD_DEV_FORCE_CHAINS)
    xp, _ = _walk(plan, m, x, st)
    assert (c1, c2) == (1, 2) and torch.isfinite(xg).all() and not torch.equal(xg, xp)
    assert torch.equal(xg, xe), "graph replay differs from eager launches"
    assert torch.equal(x2, xg), "two chains differ from one"
    # DD_NOISE_NONE: neither c z, kb z2 nor jc z3 is added
    xn, _ = _walk(plan, m, x, st, noise="none")
    xn2, _ = _walk(plan, m, x, st, noise="none", seed=77, use_graph=False)
    assert torch.equal(xn, xn2) and not torch.equal(xn, xp)


@pytest.mark.parametrize("cuts", [(3,), (4,), (3, 4), (8, 9), (1, 3, 4, 8, 9, 11)], ids=str)
def test_cut_walks_equal_the_uncut_walk(cuts):
    """cuts in front of a jump (3), behind it (4), and with a jump as a call's only row (3..4, 8..9); chains forced"""
    B = 6
    m = tiny_model(B)
    x, x0, mask = region_inputs(B, 35)
    plan, st = _plan("ddpm"), side_stream()
    xu, _ = _walk(plan, m, x, st, region=(x0, mask), flags=L.DD_DEV_FORCE_CHAINS)
    xc, c = _walk(plan, m, x, st, region=(x0, mask), flags=L.DD_DEV_FORCE_CHAINS, cuts=cuts)
    assert c == 2 and torch.isfinite(xu).all()
    assert torch.equal(xc, xu), "a cut walk differs from the uncut walk"


# ---- 4. no jumps ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_region", [False, True])
def test_walk_without_jumps_equals_sample_affine(with_region):
    """no jump row, no late row: switch_after rules, and the walk entry == dd_sample_affine[_region] (two models, the switch inside)"""
    from duodiff_amd import engine
    from duodiff_amd import step_plan as sp
    B = 6
    first, late = tiny_model(B, seed=41, depth=1), tiny_model(B, seed=42)
    x, x0, mask = region_inputs(B, 36)
    plan, st = sp.step_plan(None, use_ddim=True, ddim_steps=7, ddim_eta=0.01), side_stream()
    r = plan.rows
    rows = dict(r, jump=np.zeros(6, np.int32))
    region = (x0, mask) if with_region else None
    xw, _ = _walk(plan, first, x, st, late=late, region=region, rows=rows, switch_after=2, flags=L.DD_DEV_FORCE_CHAINS)
    xa = x.clone()
    with dev_flags(first.ctx, L.DD_DEV_FORCE_CHAINS), torch.cuda.stream(st):
        known = (known_region(plan, x0, mask),) if with_region else ()
        (engine.sample_affine_region_loop if with_region else engine.sample_affine_loop)(
            first.ctx, first, late, xa, *known, r["t"], r["a"], r["b"], r["c"], r["noise"], switch_after=2, seed=5, stream=st)
        st.synchronize()
    assert torch.isfinite(xw).all() and torch.equal(xw, xa)
    # ... and a late row that says the same is the same
    rows["late"] = (np.arange(6) >= 2).astype(np.int32)
    xl, _ = _walk(plan, first, x, st, late=late, region=region, rows=rows, flags=L.DD_DEV_FORCE_CHAINS)
    x1, _ = _walk(plan, first, x, st, region=region, rows=dict(r, jump=np.zeros(6, np.int32)))
    assert torch.equal(xl, xa) and not torch.equal(x1, xa), "the late model changed nothing"


# ---- 5. two models ----------------------------------------------------------------------------------------------------------------
def test_a_jump_across_the_switch_returns_to_the_first_model():
    """t_switch = 500 on the 6-step DDIM grid: the late model has positions 4 and 5, the jump 5 -> 3 crosses the boundary upward and
    position 3 runs the first model again.  == the steps with the model chosen per row; != the run that stays on the late model."""
    B = 6
    first, late = tiny_model(B, seed=41, depth=1), tiny_model(B, seed=42)
    x, x0, mask = region_inputs(B, 37)
    plan, st = _plan("ddim", has_late=True, t_switch=500), side_stream()
    assert plan.rows["late"].tolist() == [0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 1]
    for region in (None, (x0, mask)):
        xw, c = _walk(plan, first, x, st, late=late, region=region, flags=L.DD_DEV_FORCE_CHAINS)
        xs = _step_by_step(plan, first, x, st, late=late, region=region)
        xl = _step_by_step(plan, first, x, st, late=late, region=region, sticky_late=True)
        assert c == 2 and torch.isfinite(xw).all()
        assert torch.equal(xw, xs), "the walk differs from the steps with the model chosen per row"
        assert not torch.equal(xw, xl), "the walk equals the run that stays on the late model"
    total, t_first, t_late = first.ctx.last_sample_timing()
    assert total > 0 and t_first > 0 and t_late > 0 and abs(t_first + t_late - total) <= 1e-3 * total       # ev[1]: in front of the first late step


# ---- 6. independence and spread -----------------------------------------------------------------------------------------------------
def test_z3_is_independent_of_z_and_z2():
    """z3 differs from z and from z2 at the same counter; over the 3 072 values of 8 counters |corr| <= 5 / sqrt(N) against each
    (independent normals: a standard deviation of 1 / sqrt(N)); mean and variance of z3 within 5 standard errors of (0, 1)."""
    B = 2
    m = tiny_model(B)
    x, _, _ = region_inputs(B, 38)
    st = side_stream()
    zs, z2s, z3s = [], [], []
    for k in range(8):
        z, z2, z3 = philox_z(m, x, k, 9, st), philox_z2(m, x, k, 9, st), philox_z3(m, x, k, 9, st)
        assert not torch.equal(z3, z) and not torch.equal(z3, z2)
        for acc, v in ((zs, z), (z2s, z2), (z3s, z3)):
            acc.append(v.cpu().numpy().ravel())
    a, b, c = (np.concatenate(v).astype(np.float64) for v in (zs, z2s, z3s))
    n = c.size
    assert n == 3072
    r1, r2 = float(np.corrcoef(c, a)[0, 1]), float(np.corrcoef(c, b)[0, 1])
    print(f"corr(z3, z) {r1:.4f}, corr(z3, z2) {r2:.4f} over {n} values (bound {5 / np.sqrt(n):.4f}); z3 mean {c.mean():.4f} var {c.var():.4f}")
    assert abs(r1) <= 5 / np.sqrt(n) and abs(r2) <= 5 / np.sqrt(n)
    assert abs(c.mean()) <= 5 / np.sqrt(n) and abs(c.var() - 1) <= 5 * np.sqrt(2 / n)
    assert np.array_equal(philox_z3(m, x, 3, 9, st).cpu().numpy().ravel(), z3s[3])          # a pure function of (seed, pixel, counter)
    assert not np.array_equal(philox_z3(m, x, 3, 10, st).cpu().numpy().ravel(), z3s[3])


# ---- 7. replay and poison ---------------------------------------------------------------------------------------------------------
def test_second_call_replays_the_graphs():
    """A second call with other tensors of the same shape gives that call's own result and captures nothing: the step's graph and the
    jump's are replayed."""
    B = 2
    m = tiny_model(B)
    plan, st = _plan("ddim"), side_stream()
    x, x0a, ma = region_inputs(B, 39)
    xb, x0b, _ = region_inputs(B, 40)
    mb = (1 - ma).contiguous()
    lib, h = m.ctx.lib, m.ctx.handle
    n_before = lib.dd_dev_graph_captures(h)
    ra, _ = _walk(plan, m, x, st, region=(x0a, ma))
    n0 = lib.dd_dev_graph_captures(h)
    assert n0 >= n_before + 1        # (the step's graph is the model's; the jump's is the context's and may be there already)
    rb, _ = _walk(plan, m, xb, st, region=(x0b, mb))
    assert lib.dd_dev_graph_captures(h) == n0, "the second call re-captured a graph"
    sa, sb = _step_by_step(plan, m, x, st, region=(x0a, ma)), _step_by_step(plan, m, xb, st, region=(x0b, mb))
    assert torch.equal(ra, sa) and torch.equal(rb, sb) and not torch.equal(ra, rb)
    ra2, _ = _walk(plan, m, x, st, region=(x0a, ma))
    assert torch.equal(ra2, ra)


def test_poisoned_workspaces_change_nothing():
    """Both chains' workspaces NaN-poisoned before the call, on fresh models: == the clean run (chains forced)."""
    B = 6
    x, x0, mask = region_inputs(B, 41)
    plan, st = _plan("ddim"), side_stream()
    outs = []
    for poison in (False, True):
        m = tiny_model(B, seed=71)
        if poison:
            m.ctx.check(m.ctx.lib.dd_dev_poison_workspaces(m.ctx.handle, m.handle, st.cuda_stream))
        outs.append(_walk(plan, m, x, st, region=(x0, mask), flags=L.DD_DEV_FORCE_CHAINS))
        del m
    assert outs[0][1] == outs[1][1] == 2 and torch.isfinite(outs[0][0]).all()
    assert torch.equal(outs[0][0], outs[1][0]), "poisoned run differs"


# ---- 8. rejections ----------------------------------------------------------------------------------------------------------------
def test_invalid_walk_calls_are_rejected_before_anything_is_enqueued():
    from duodiff_amd.engine import Model
    B = 2
    m, guide = tiny_model(B), tiny_model(B, seed=41, depth=1)
    ctx, lib = m.ctx, m.ctx.lib
    ee = Model(ctx, ModelParams.from_dict(dict(TINY)), B)
    ee.enable_early_exit("mlp_probe_per_layer")
    x_in, x0, mask = region_inputs(B, 42)
    st = side_stream()
    plan = _plan("ddim")
    tab = {k: np.ascontiguousarray(v[2:5]) for k, v in plan.rows.items()}         # a step, the jump, a step
    assert tab["jump"].tolist() == [0, 1, 0]
    ka, kb = np.ones(3, np.float32), np.zeros(3, np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    n0 = lib.dd_dev_graph_captures(ctx.handle)
    cases = [("null_walk", "dd_walk"), ("null_jump", "jump array"), ("jump_b", "b != 0"), ("late_range", "outside {0, 1}"),
             ("late_without_model", "without a late model"), ("both", "exclusive"), ("both_region", "exclusive"), ("early_exit", "early-exit"),
             ("early_exit_region", "early-exit"), ("host_noise", "noise"), ("host_noise_region", "noise"), ("null_region_member", "member"),
             ("x_null", "null tensor"), ("batch", "batch size")]
    for what, msg in cases:
        x = x_in.clone()
        a = L.dd_affine_sample_args()
        a.first, a.late, a.n_steps, a.switch_after = (ee if what.startswith("early_exit") else m).handle, None, 3, 3
        b = tab["b"].copy()
        if what == "jump_b":
            b[1] = 0.25
        for k, v in dict(tab, b=b).items():
            if k in "tabc":
                setattr(a, k, fp(v))
        a.noise = ip(tab["noise"])
        a.noise_mode = L.DD_NOISE_BUFFER if what.startswith("host_noise") else L.DD_NOISE_PHILOX
        a.use_graph, a.seed, a.B, a.y_dev = 1, 1, (B + 1 if what == "batch" else B), None
        a.x_dev = None if what == "x_null" else x.data_ptr()
        late_row = np.array([0, 0, {"late_range": 2, "late_without_model": 1}.get(what, 0)], np.int32)
        walk = L.dd_walk(None if what == "null_jump" else ip(tab["jump"]), ip(late_row))
        kr = L.dd_known_region(None if what == "null_region_member" else x0.data_ptr(), mask.data_ptr(), fp(ka), fp(kb))
        with_region = what.endswith("_region") or what == "null_region_member"
        g = L.dd_guidance(0.5, NULL) if what.startswith("both") else None
        ag = L.dd_autoguidance(guide.handle, 0.5) if what.startswith("both") else None
        with torch.cuda.stream(st):
            rc = lib.dd_sample_affine_walk(ctx.handle, C.byref(a), None if g is None else C.byref(g), None if ag is None else C.byref(ag),
                                           C.byref(kr) if with_region else None, None if what == "null_walk" else C.byref(walk),
                                           C.c_void_p(st.cuda_stream))
        st.synchronize()
        err = lib.dd_last_error(ctx.handle).decode()
        print(f"{what}: rc {rc}, {err!r}")
        assert rc == L.DD_ERR_INVALID and msg in err, (what, rc, err)
        assert torch.equal(x, x_in), f"{what}: something was enqueued"
    assert lib.dd_dev_graph_captures(ctx.handle) == n0
    # the order of the walk's own checks: a null walk before a bad row, a bad row before the two guidances, those before the noise mode
    a.x_dev, a.B, a.noise_mode = x.data_ptr(), B, L.DD_NOISE_BUFFER
    b = tab["b"].copy()
    b[1] = 0.25
    a.b = fp(b)
    g, ag = L.dd_guidance(0.5, NULL), L.dd_autoguidance(guide.handle, 0.5)
    walk = L.dd_walk(ip(tab["jump"]), None)
    for w, want in ((None, "null dd_walk / null jump array"), (C.byref(walk), "row 1 is a jump with b != 0: a jump runs no model")):
        rc = lib.dd_sample_affine_walk(ctx.handle, C.byref(a), C.byref(g), C.byref(ag), None, w, C.c_void_p(st.cuda_stream))
        assert rc == L.DD_ERR_INVALID and lib.dd_last_error(ctx.handle).decode() == want
    a.b = fp(tab["b"])
    rc = lib.dd_sample_affine_walk(ctx.handle, C.byref(a), C.byref(g), C.byref(ag), None, C.byref(walk), C.c_void_p(st.cuda_stream))
    assert rc == L.DD_ERR_INVALID and lib.dd_last_error(ctx.handle).decode() == "classifier-free guidance and autoguidance are exclusive"
    from duodiff_amd import engine
    with pytest.raises(ValueError, match="perturbed-attention"):
        engine.sample_affine_walk_loop(ctx, m, None, x, plan.rows, guidance=engine.Perturbed(1.0, [1]))
    st.synchronize()
    assert torch.equal(x, x_in)


# ---- 9. the oracle ----------------------------------------------------------------------------------------------------------------
def test_fp32_engine_matches_the_oracle_over_the_walk():
    """The (6, 2, 2) DDIM walk with the left half of the image known: the fp32 engine (device loop) against the numpy oracle driven by
    the extracted z / z2 / z3, the rules restated in float64.  max abs <= 1e-3, the region test's bound: a jump multiplies both sides by
    ja <= 1 and adds the same jc z3, so it cannot widen the gap.  Measured on MI355X: see DESIGN.md section 7l."""
    import oracle
    from duodiff_amd import step_plan as sp
    B = 3
    cfg = dict(TINY)
    mp = ModelParams.from_dict(cfg)
    sd = synthetic_state_dict(mp, 61)
    orc = oracle.UViTOracle(mp.as_dict(), {k: v.numpy() for k, v in sd.items()})
    em = uvit(cfg, 61, "fp32", B)[0].engine_model(B)
    plan = _plan("ddim")
    ka, kb = sp.known_rows(plan)
    xd, x0, mask = region_inputs(B, 62, mask="half")
    st = side_stream()
    x, k0, mk = xd.cpu().numpy().astype(np.float64), x0.cpu().numpy().astype(np.float64), mask.cpu().numpy().astype(np.float64)
    r = plan.rows
    for k in range(len(r["t"])):
        if r["jump"][k]:
            x = float(r["a"][k]) * x + float(r["c"][k]) * philox_z3(em, xd, k, 5, st).cpu().numpy().astype(np.float64)
            continue
        eps = orc(x.astype(np.float32), np.full((B,), float(r["t"][k]), np.float32)).astype(np.float64)
        v = float(r["a"][k]) * x + float(r["b"][k]) * eps
        if r["noise"][k]:
            v = v + float(r["c"][k]) * philox_z(em, xd, k, 5, st).cpu().numpy().astype(np.float64)
        kn = float(ka[k]) * k0
        if kb[k] != 0:
            kn = kn + float(kb[k]) * philox_z2(em, xd, k, 5, st).cpu().numpy().astype(np.float64)
        x = np.where(mk == 0, v, mk * kn + (1 - mk) * v)
    got, _ = _walk(plan, em, xd, st, region=(x0, mask))
    err = float(np.abs(got.cpu().numpy() - x).max())
    print(f"fp32 engine vs the oracle, the (6, 2, 2) DDIM walk with a half-image mask: max abs {err:.3e} (|x| max {np.abs(x).max():.3f})")
    assert np.isfinite(err) and err <= 1e-3
    assert np.array_equal(got.cpu().numpy()[..., :4], x0.cpu().numpy()[..., :4])


# ---- 10. full width ---------------------------------------------------------------------------------------------------------------
def test_celeba_width_two_real_chains():
    """embed_dim 512, depth 3, 64 x 64, B = 32 in bf16: the (4, 2, 2) DDIM walk with a region as two real chains == one chain, and the
    known pixels are the known image."""
    from duodiff_amd import step_plan as sp
    B = 32
    m = uvit(load_config(CELEBA_3), 51, "bf16", B)[0].engine_model(B)
    x, x0, mask = region_inputs(B, 43, S=64)
    plan = sp.step_plan("predict_noise", use_ddim=True, ddim_steps=5, ddim_eta=0.01, resample_jump=2, resample_count=2)
    assert [mv[0] for mv in plan.moves] == ["S", "S", "S", "J", "S", "S", "S"]
    st = side_stream()
    x2, c2 = _walk(plan, m, x, st, region=(x0, mask))
    x1, c1 = _walk(plan, m, x, st, region=(x0, mask), flags=L.DD_DEV_NO_CHAINS)
    assert (c2, c1) == (2, 1) and torch.isfinite(x2).all()
    assert torch.equal(x2, x1), "two real chains differ from one"
    keep = (mask == 1).expand_as(x0)
    assert torch.equal(x2[keep], x0[keep])


# ---- 11. end to end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", ["device", "torch_cpu"])
def test_cli_resampling_end_to_end(tmp_path, noise):
    """--resample_jump / --resample_count with --known_image / --known_mask: the files are written and the known pixels of samples.npy
    equal (x0 + 1) / 2."""
    import yaml
    cfg = dict(TINY)
    (tmp_path / "m.yaml").write_text(yaml.safe_dump({"model_params": cfg}))
    torch.save(dict(synthetic_state_dict(ModelParams.from_dict(cfg), 91)), tmp_path / "m.pth")
    rng = np.random.default_rng(1)
    x0 = rng.uniform(-1, 1, (1, 3, 8, 8)).astype(np.float32)
    mask = np.zeros((3, 1, 8, 8), np.float32)
    mask[:, :, 2:6, 1:7] = 1
    mask[1] = 1 - mask[1]
    np.save(tmp_path / "x0.npy", x0)
    np.save(tmp_path / "mask.npy", mask)
    out = tmp_path / "out"
    cmd = [sys.executable, "-m", "duodiff_amd.sampler", "--seed", "5", "--checkpoint_path", str(tmp_path / "m.pth"),
           "--config_path", str(tmp_path / "m.yaml"), "--batch_size", "3", "--parametrization", "predict_noise", "--output_folder", str(out),
           "--no_png", "--use_ddim", "--ddim_steps", "7", "--noise", noise, "--resample_jump", "2", "--resample_count", "2",
           "--known_image", str(tmp_path / "x0.npy"), "--known_mask", str(tmp_path / "mask.npy")]
    r = subprocess.run(cmd, cwd=str(REPO), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert (out / "statistics.txt").exists()
    s = np.load(out / "samples.npy")
    assert s.shape == (3, 8, 8, 3) and np.isfinite(s).all()
    want = np.broadcast_to(((x0 + np.float32(1)) / np.float32(2)).transpose(0, 2, 3, 1), s.shape)
    keep = np.broadcast_to(mask.transpose(0, 2, 3, 1) == 1, s.shape)
    assert np.array_equal(s[keep], want[keep])
    assert not np.array_equal(s[~keep], want[~keep])


def test_get_samples_walks_on_the_device_and_on_the_host():
    """get_samples with resample_jump / resample_count: the device run is the walk loop cut at the save (== the rows run as one call), the
    intermediate is the LAST visit's x, Restart runs, and r = 1 is the run without the arguments."""
    from duodiff_amd import sampler
    model = uvit(dict(TINY), 91, "bf16", 3)[0]
    kw = dict(model=model, batch_size=3, postprocessing=sampler.predict_noise_postprocessing, seed=5, num_channels=3, sample_height=8,
              sample_width=8, use_ddim=True, ddim_steps=7, ddim_eta=0.01, noise="device", return_device_tensor=True)
    plain, _ = sampler.get_samples(**kw)
    same, _ = sampler.get_samples(**kw, resample_jump=2, resample_count=1)
    walked, inter = sampler.get_samples(**kw, resample_jump=2, resample_count=2, timesteps_save=[501])
    uncut, _ = sampler.get_samples(**kw, resample_jump=2, resample_count=2)
    assert torch.equal(same, plain) and not torch.equal(walked, plain) and torch.isfinite(walked).all()
    assert torch.equal(walked, uncut) and len(inter) == 1, "the save cut the walk visibly"
    plan = _plan("ddim", timesteps_save=[501])
    assert [k for k, s in enumerate(plan.save_after) if s] == [9]
    em, st = model.engine_model(3), side_stream()
    sampler.seed_everything(5)
    x = torch.randn(3, 3, 8, 8).cuda().contiguous()
    upto = plan._replace(rows={k: v[:10] for k, v in plan.rows.items()})
    x9, _ = _walk(upto, em, x, st, rows=upto.rows)
    assert np.array_equal(inter[0], em.ctx.to_images(x9.contiguous()).cpu().numpy())
    restarted, _ = sampler.get_samples(**kw, restart=[(100, 500, 2)])
    assert torch.isfinite(restarted).all() and not torch.equal(restarted, plain)
    host, _ = sampler.get_samples(**dict(kw, noise="torch_cpu"), resample_jump=2, resample_count=2)
    assert torch.isfinite(host).all() and not torch.equal(host, walked)
