"""x0 clipping and dynamic thresholding of the multistep loop: the unfolded rows, the rule against its numpy
float32 restatement bit for bit, the device loop against the composition of its parts, graph keys, cuts, poison, and the fp32 engine
against a float64 restatement on the numpy oracle."""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch

from conftest import REPO, TINY
from duodiff_amd import _lib as L
from duodiff_amd.config import ModelParams
from duodiff_amd.weights import synthetic_state_dict
from kernel_support import step_history, step_table
from loop_support import NULL, cli_argv, images, labels, run_loop, run_steps, side_stream, tiny_model, uvit

gpu = pytest.mark.gpu
CELEBA, IMAGENET256 = REPO / "configs" / "uvit_celeba.yaml", REPO / "configs" / "uvit_imagenet256.yaml"
F = np.float32


def _thr(mode, **kw):
    from duodiff_amd.engine import X0Threshold
    return X0Threshold(mode, **kw)


# ---- the rule, restated in numpy: every product and sum rounded to float32 on its own, in the order of include/duodiff.h; the update and
# the history are kernel_support's restatement of step_update.h, shared with tests/test_final_step.py ----------
def _scale(x0_image, qt, smax, dtype=F):
    """s of one image; dtype float64: the same expression without the float32 roundings"""
    v = np.sort(np.abs(x0_image).ravel())
    n = v.size
    pos = np.float64(F(qt)) * np.float64(n - 1)
    i = int(np.floor(pos))
    f = dtype(F(pos - i))
    with np.errstate(invalid="ignore", over="ignore"):
        s = dtype(v[i]) + f * (dtype(v[min(i + 1, n - 1)]) - dtype(v[i]))
        return dtype(min(max(s, dtype(1)), dtype(smax)))


def _restate(x, m, z, h, thr, a, b, c, d, p, q, use_hist, dtype=F):
    x, m = np.asarray(x, dtype), np.asarray(m, dtype)
    a, b, c, d, p, q = (dtype(v) for v in (a, b, c, d, p, q))
    with np.errstate(invalid="ignore", over="ignore"):
        x0 = step_history(x, m, p, q, dtype)
        if thr.mode == "static":
            r = dtype(F(thr.range))
            xh = np.minimum(np.maximum(x0, -r), r)
        else:
            xh = np.empty_like(x0)
            for i in range(len(x0)):
                s = _scale(x0[i], thr.quantile, F(thr.s_max), dtype)
                xh[i] = np.minimum(np.maximum(x0[i], -s), s) / s
    return step_table(x, xh, z, h, a, b, c, d, use_hist, dtype), xh


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def _tables64():
    from duodiff_amd.engine import schedule_tables
    return {k: v.astype(np.float64) for k, v in schedule_tables().items()}


def test_unfolded_and_folded_rows_agree_in_float64():
    from duodiff_amd import sampler
    tb = _tables64()
    ab = tb["alphas_bar"]

    def close(u, a_f, b_f, ok=slice(None)):
        np.testing.assert_allclose((u["a"] + u["b"] * u["p"])[ok], a_f[ok], rtol=1e-12, atol=0)
        np.testing.assert_allclose((u["b"] * u["q"])[ok], b_f[ok], rtol=1e-12, atol=0)

    for kind in sampler.MULTISTEP_KINDS:
        for par in ("predict_noise", "predict_original"):
            for order in (1, 2):
                grid = ab[sampler.multistep_grid(20)]
                fo, un = sampler.multistep_rows(kind, grid, order, par), sampler.multistep_rows(kind, grid, order, par, unfolded=True)
                close(un, fo["a"], fo["b"])
                for k in ("c", "d", "p", "q", "hist", "noise"):
                    assert np.array_equal(fo[k], un[k]), k
    ts = np.linspace(0, 999, 50).astype(int)[::-1]
    t, s = ts[:-1], ts[1:]
    for eta in (0.0, 1.0):      # the reference's DDIM (sampler.py:112-120) in float64: a = sqrt(abar_s / abar_t), b = dir - a sqrt(1 - abar_t)
        un = sampler.unfolded_rows("ddim", ts, eta)
        sig2 = tb["betas_tilde"][t] * eta
        a_f = np.sqrt(ab[s] / ab[t])
        with np.errstate(invalid="ignore"):
            dirn = np.sqrt(1 - ab[s] - sig2)
        # (eta = 1, the step onto t = 0: 1 - abar_0 < betas_tilde[t], the reference's own direction term is NaN there, and so are the rows)
        ok = np.isfinite(dirn)
        assert ok[:-1].all() and (ok[-1] or eta == 1.0) and np.array_equal(np.isfinite(un["a"]), ok)
        close(un, a_f, dirn - a_f * np.sqrt(1 - ab[t]), ok)
        assert np.array_equal(un["c"], sig2) and np.array_equal(un["noise"], (s > 0).astype(np.int32)) and not un["hist"].any()
    # ancestral DDPM: the posterior mean (sampler.py:59-72) with x0 = (x - sqrt(1 - abar) eps) / sqrt(abar) folded in, as one fraction
    # over the same table entries (the float32 tables satisfy abar_t = alpha_t abar_{t-1} only to their own rounding, so the textbook
    # 1 / sqrt(alpha_t) is not the float64 fold of these rows)
    t = np.arange(999, -1, -1)
    un = sampler.unfolded_rows("ddpm", t)
    al, abp, be = tb["alphas"][t], tb["alphas_bar_previous"][t], tb["betas"][t]
    close(un, (np.sqrt(al) * (1 - abp) * np.sqrt(ab[t]) + np.sqrt(abp) * be) / ((1 - ab[t]) * np.sqrt(ab[t])),
          -np.sqrt(abp) * be * np.sqrt(1 - ab[t]) / ((1 - ab[t]) * np.sqrt(ab[t])))
    assert not un["hist"].any() and np.array_equal(un["noise"], (t > 0).astype(np.int32))
    un = sampler.unfolded_rows("ddpm", t, parametrization="predict_original")
    assert np.array_equal(un["p"], np.zeros(1000)) and np.array_equal(un["q"], np.ones(1000))
    for k, (a, b, c) in ((999, sampler.affine_coefficients("predict_original", 999)), (3, sampler.affine_coefficients("predict_original", 3))):
        i = 999 - k
        np.testing.assert_allclose([un["a"][i], un["b"][i], un["c"][i]], [a, b, c], rtol=1e-6)


def test_default_rows_are_byte_identical_to_the_folded_rows_of_the_parent():
    """sha256 over the default multistep_coefficients of the argument sets tests/test_multistep.py uses, recorded on the parent commit"""
    from duodiff_amd import sampler
    hsh = hashlib.sha256()
    for kind in sampler.MULTISTEP_KINDS:
        for par in ("predict_noise", "predict_original"):
            for order in (1, 2):
                for n in (6, 10, 20):
                    r = sampler.multistep_coefficients(kind, sampler.multistep_grid(n), order, par)
                    r2 = sampler.multistep_coefficients(kind, sampler.multistep_grid(n), order, par, unfolded=False)
                    for k in sorted(r):
                        hsh.update(np.ascontiguousarray(r[k]).tobytes())
                        assert r[k].tobytes() == r2[k].tobytes()
    assert hsh.hexdigest() == "4928b93c5b57b31d22bab7cca4ce95274449d2d9c8030d78c7a5efd1d350f681"


@pytest.mark.parametrize("kind", ["dpmsolver++", "sde-dpmsolver++"])
def test_restatement_with_a_huge_range_reproduces_the_folded_step(kind):
    """range = 3e38 clips nothing: unfolded rows through the rule == the folded multistep step within 4 ulp of |a x| + |b m| + |d h|"""
    from duodiff_amd import sampler
    g = np.random.default_rng(3)
    ts = sampler.multistep_grid(6)
    fo, un = sampler.multistep_coefficients(kind, ts, 2), sampler.multistep_coefficients(kind, ts, 2, unfolded=True)
    x, m, h, z = (g.standard_normal((2, 3, 8, 8)).astype(F) for _ in range(4))
    worst = 0.0
    for k in range(6):
        got, _ = _restate(x, m, z if un["noise"][k] else None, h, _thr("static", range=3e38), *(un[c][k] for c in "abcdpq"), un["hist"][k])
        want = fo["a"][k] * x + fo["b"][k] * m
        mag = np.abs(fo["a"][k] * x) + np.abs(fo["b"][k] * m)
        if fo["hist"][k]:
            want, mag = want + fo["d"][k] * h, mag + np.abs(fo["d"][k] * h)
        if fo["noise"][k]:
            want = want + fo["c"][k] * z
        assert want.dtype == F and got.dtype == F
        ulps = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(mag).astype(np.float64)
        worst = max(worst, float(ulps.max()))
    print(f"{kind}: unfolded through the rule vs folded, worst {worst:.2f} ulp of |a x| + |b m| + |d h|")
    assert worst <= 4.0


@pytest.mark.parametrize("qt", [1e-4, 0.5, 0.995, 1.0])
def test_restated_scale_against_numpy_quantile(qt):
    g = np.random.default_rng(4)
    for n, sigma in ((192, 3.0), (768, 160.0), (16384, 3.0), (4096, 1.5)):
        x0 = (g.standard_normal(n) * sigma).astype(F)
        s = _scale(x0, qt, np.inf)
        want = max(np.quantile(np.abs(x0).astype(np.float64), np.float64(F(qt))), 1.0)
        assert abs(np.float64(s) - want) <= np.spacing(F(want)), (n, sigma, s, want)


def _argv(*extra, config=CELEBA, par="predict_noise"):
    return cli_argv(config, *extra, par=par)


def test_cli_threshold_options():
    from duodiff_amd import sampler
    from duodiff_amd.config import load_config
    cfg = load_config(CELEBA)
    a = sampler.get_args(_argv())
    assert a.clip_x0 is None and a.dynamic_threshold is None and a.threshold_max is None and sampler.validate_threshold(a, cfg) is None
    assert sampler.validate_threshold(sampler.get_args(_argv("--clip_x0")), cfg) == _thr("static", range=1.0)
    assert sampler.validate_threshold(sampler.get_args(_argv("--clip_x0", "0.5")), cfg) == _thr("static", range=0.5)
    t = sampler.validate_threshold(sampler.get_args(_argv("--dynamic_threshold", "0.995", "--threshold_max", "2")), cfg)
    assert t == _thr("dynamic", quantile=0.995, s_max=2.0)
    assert sampler.validate_threshold(sampler.get_args(_argv("--dynamic_threshold", "0.9")), cfg).s_max == np.inf
    for extra in (["--cfg_scale", "2", "--class_label", "1"], ["--autoguidance_scale", "1"], ["--use_ddim"], ["--dpm_solver", "sde"],
                  ["--timesteps_save", "500"], ["--t_switch", "300"], ["--init_image", "a.npy", "--strength", "0.5"],
                  ["--known_image", "a.npy", "--known_mask", "m.npy"]):
        assert sampler.validate_threshold(sampler.get_args(_argv("--clip_x0", *extra)), cfg) is not None


@pytest.mark.parametrize("extra,kw,match", [
    (["--clip_x0", "--dynamic_threshold", "0.9"], {}, "exclusive"),
    (["--clip_x0", "0"], {}, "positive"),
    (["--clip_x0", "inf"], {}, "finite"),
    (["--dynamic_threshold", "0"], {}, "outside"),
    (["--dynamic_threshold", "1.5"], {}, "outside"),
    (["--dynamic_threshold", "0.9", "--threshold_max", "0.5"], {}, "at least 1"),
    (["--threshold_max", "2"], {}, "goes with"),
    (["--clip_x0", "--threshold_max", "2"], {}, "goes with"),
    (["--clip_x0"], dict(config=IMAGENET256), "latent"),
    (["--dynamic_threshold", "0.9"], dict(par="predict_previous"), "predict_previous"),
    (["--clip_x0", "--noise", "torch_cpu"], {}, "--noise device"),
])
def test_cli_rejects_invalid_threshold_options_before_any_gpu_work(tmp_path, monkeypatch, extra, kw, match):
    from duodiff_amd import engine, sampler

    def no_engine(*a, **k):
        raise AssertionError("an engine context was created")
    monkeypatch.setattr(engine.Context, "__init__", no_engine)
    argv = _argv(*extra, **kw)
    argv[argv.index("--output_folder") + 1] = str(tmp_path / "out")
    with pytest.raises(ValueError, match=match):
        sampler.main(argv)


def test_step_plan_with_a_threshold():
    from duodiff_amd import sampler
    thr = _thr("static")
    for kw in (dict(solver="dpmsolver++", solver_steps=6), dict(solver="sde-dpmsolver++", solver_steps=6), dict(use_ddim=True, ddim_steps=7),
               dict(num_steps=12)):
        for par in ("predict_noise", "predict_original"):
            plain, plan = sampler.step_plan(par, **kw), sampler.step_plan(par, threshold=thr, **kw)
            assert plan.kind == "multistep" and set(plan.rows) == set("tabcdpq") | {"hist", "noise"}
            assert np.array_equal(plan.rows["t"], plain.rows["t"]) and np.array_equal(plan.rows["noise"], plain.rows["noise"])
            assert plan.lands == plain.lands and plan.save_after == plain.save_after and plan.switch_after == plain.switch_after
            assert all(v.dtype == (np.int32 if k in ("hist", "noise") else F) for k, v in plan.rows.items())
        with pytest.raises(ValueError, match="predict_previous"):
            sampler.step_plan("predict_previous", threshold=thr, **kw)
    un = sampler.step_plan("predict_noise", threshold=thr, solver="dpmsolver++", solver_steps=6).rows
    ref = sampler.multistep_coefficients("dpmsolver++", sampler.multistep_grid(6), 2, unfolded=True)
    assert all(np.array_equal(un[k], ref[k]) for k in ref)
    assert sampler.step_plan("predict_noise", solver="dpmsolver++", solver_steps=6).rows["a"].tobytes() != un["a"].tobytes()


def test_lib_binds_the_threshold_entry_points():
    assert L.ABI_VERSION == 6 and (L.DD_X0_STATIC, L.DD_X0_DYNAMIC) == (0, 1)
    assert C.sizeof(L.dd_x0_threshold) == 16 and [f[0] for f in L.dd_x0_threshold._fields_] == ["mode", "quantile", "range", "s_max"]
    assert len(L.SIGNATURES["dd_threshold_step"][1]) == 18 and L.SIGNATURES["dd_threshold_step"][1][5] == C.POINTER(L.dd_x0_threshold)
    assert L.SIGNATURES["dd_sample_multistep_threshold"][1] == [
        C.c_void_p, C.POINTER(L.dd_multistep_sample_args), C.POINTER(L.dd_guidance), C.POINTER(L.dd_autoguidance),
        C.POINTER(L.dd_known_region), C.POINTER(L.dd_x0_threshold), C.c_void_p]
    lib = L.load()
    assert hasattr(lib, "dd_threshold_step") and hasattr(lib, "dd_sample_multistep_threshold")


# ---- GPU: dd_threshold_step against the restatement, bit for bit ---------------------------------------------------------------------
SHAPES = [(3, 3, 8), (5, 3, 16), (2, 4, 32), (2, 3, 64), (1, 4, 64)]
CO = dict(a=0.9813, b=-0.2371, c=0.0417, d=-0.5333)


def _inputs(shape, seed):
    """name -> x0 [B, C, S, S] float32; the step runs on x = x0, p = 1, q = 0 and m = -1 (q m = -0, so x0 = x to the bit, -0 included)"""
    g = np.random.default_rng(seed)
    B, n = shape[0], int(np.prod(shape[1:]))
    out = {f"gauss{s}": (g.standard_normal(shape) * s).astype(F) for s in (0.3, 3.0, 160.0)}
    out["quantised"] = (np.round(g.standard_normal(shape) * 8) * 0.25).astype(F)
    eq = (g.standard_normal(shape) * 2).astype(F)
    eq[0] = F(-1.75)
    out["one_image_equal"] = eq
    mix = (g.standard_normal(shape) * 10.0 ** g.uniform(-40, 30, shape)).astype(F)
    assert ((np.abs(mix) < 1.17e-38) & (mix != 0)).any() and np.isfinite(mix).all()
    mix.reshape(B, n)[:, :4] = [0.0, -0.0, 1e-45, -1e-45]
    out["mixed_magnitudes"] = mix
    inf = (g.standard_normal(shape) * 3).astype(F)
    inf.reshape(B, n)[0, n // 3] = np.inf
    out["one_inf"] = inf
    return out


def _run_step(ctx, x, m, z, h, thr, co, use_hist, out=None):
    o = ctx.threshold_step(x, m, z, h, thr, co["a"], co["b"], co["c"], co["d"], co["p"], co["q"], use_hist, out=out)
    torch.cuda.synchronize()
    return o


def _same_bits(got, want):
    return np.array_equal(np.asarray(got).view(np.uint32), np.asarray(want).view(np.uint32))


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_threshold_step_equals_the_restatement_bit_for_bit(shape):
    from duodiff_amd.engine import Context
    ctx = Context.get()
    B, C_, S = shape
    full = (B, C_, S, S)
    g = np.random.default_rng(7)
    co = dict(CO, p=1.0, q=0.0)
    z, h = (g.standard_normal(full).astype(F) for _ in range(2))
    m = np.full(full, -1.0, F)
    zd, md = torch.from_numpy(z).cuda(), torch.from_numpy(m).cuda()
    thresholds = [_thr("dynamic", quantile=qt, s_max=sm) for qt in (1e-4, 0.5, 0.995, 1.0) for sm in (np.inf, 2.0)]
    thresholds += [_thr("static", range=r) for r in (1.0, 0.5)]
    ran = 0
    for name, x0 in _inputs(full, 11).items():
        for thr in thresholds:
            if name == "one_inf" and not (thr.mode == "dynamic" and thr.quantile == 0.5):
                continue
            if thr.mode == "static":
                x0 = x0.copy()
                x0.reshape(B, -1)[:, 5:9] = [thr.range, -thr.range, np.nextafter(F(thr.range), F(9)), -np.nextafter(F(thr.range), F(0))]
            for use_hist, with_z in ((1, True), (0, False)) if ran % 2 else ((1, False), (0, True)):
                # without history h is NaN-filled: it never reaches x', and h' is written all the same
                hd = torch.from_numpy(h).cuda() if use_hist else torch.full(full, float("nan"), device="cuda")
                out = _run_step(ctx, torch.from_numpy(x0).cuda(), md, zd if with_z else None, hd, thr, co, use_hist)
                want, xh = _restate(x0, m, z if with_z else None, h, thr, **co, use_hist=use_hist)
                tag = (name, thr, use_hist, with_z)
                assert _same_bits(hd.cpu().numpy(), xh), ("h'", tag)
                assert _same_bits(out.cpu().numpy(), want), ("x'", tag)
                if name != "one_inf" and name != "mixed_magnitudes":
                    assert np.isfinite(out.cpu().numpy()).all(), tag
                ran += 1
            if name == "gauss0.3" and thr.mode == "dynamic" and thr.quantile <= 0.5:      # (the median of |x0| is ~0.2) every s floors to 1: xh is the clamp to [-1, 1]
                assert all(_scale(v, thr.quantile, F(thr.s_max)) == 1 for v in x0)
                assert _same_bits(xh, np.minimum(np.maximum(x0, F(-1)), F(1)) / F(1))
    # a general row: p, q of a predict_noise step at t = 999, Gaussian x and m
    co = dict(CO, p=157.41045, q=-157.40727)
    x, m2 = (g.standard_normal(full).astype(F) for _ in range(2))
    for thr in (_thr("dynamic", quantile=0.995), _thr("dynamic", quantile=0.5, s_max=2.0), _thr("static", range=1.0)):
        hd = torch.from_numpy(h).cuda()
        out = _run_step(ctx, torch.from_numpy(x).cuda(), torch.from_numpy(m2).cuda(), zd, hd, thr, co, 1)
        want, xh = _restate(x, m2, z, h, thr, **co, use_hist=1)
        assert _same_bits(out.cpu().numpy(), want) and _same_bits(hd.cpu().numpy(), xh), thr


@gpu
def test_threshold_step_images_are_independent_canaries_and_aliasing():
    from duodiff_amd.engine import Context
    ctx = Context.get()
    B, C_, S = 5, 3, 16
    n = C_ * S * S
    g = torch.Generator().manual_seed(8)
    x, m, z, h = (torch.randn(B, C_, S, S, generator=g).cuda() * sc for sc in (1.0, 1.0, 1.0, 1.0))
    x = x * torch.tensor([0.2, 1.0, 3.0, 9.0, 40.0], device="cuda").view(B, 1, 1, 1)       # another scale per image
    co = dict(CO, p=1.31, q=-0.77)
    thr = _thr("dynamic", quantile=0.9)
    # out and h live inside larger buffers whose other bytes are canaries
    pad = 64
    obuf, hbuf = (torch.full((B * n + 2 * pad,), 12345.0, device="cuda") for _ in range(2))
    out, hh = (b[pad:pad + B * n].view(B, C_, S, S) for b in (obuf, hbuf))
    hh.copy_(h)
    _run_step(ctx, x, m, z, hh, thr, co, 1, out=out)
    for buf in (obuf, hbuf):
        assert (buf[:pad] == 12345.0).all() and (buf[-pad:] == 12345.0).all(), "bytes around out / h were written"
    want, xh = _restate(x.cpu().numpy(), m.cpu().numpy(), z.cpu().numpy(), h.cpu().numpy(), thr, **co, use_hist=1)
    assert _same_bits(out.cpu().numpy(), want) and _same_bits(hh.cpu().numpy(), xh)
    for b in (0, 3, 4):
        h1 = h[b:b + 1].clone()
        o1 = _run_step(ctx, x[b:b + 1].clone(), m[b:b + 1].clone(), z[b:b + 1].clone(), h1, thr, co, 1)
        assert torch.equal(o1[0], out[b]) and torch.equal(h1[0], hh[b]), f"image {b} of B = 5 differs from its B = 1 call"
    xi, h2 = x.clone(), h.clone()      # in place
    _run_step(ctx, xi, m, z, h2, thr, co, 1, out=xi)
    assert torch.equal(xi, out) and torch.equal(h2, hh)
    # S * S no multiple of 4: the scalar-access form of the kernel
    xo, mo, zo, ho = (torch.randn(2, 3, 7, 7, generator=g).cuda() * 2 for _ in range(4))
    ho0 = ho.clone()
    oo = _run_step(ctx, xo, mo, zo, ho, thr, co, 1)
    want, xh = _restate(xo.cpu().numpy(), mo.cpu().numpy(), zo.cpu().numpy(), ho0.cpu().numpy(), thr, **co, use_hist=1)
    assert _same_bits(oo.cpu().numpy(), want) and _same_bits(ho.cpu().numpy(), xh)
    for bad, exc in ((dict(mode="dynamic", quantile=0.0), ValueError), (dict(mode="dynamic", quantile=1.5), ValueError),
                     (dict(mode="dynamic", s_max=0.5), ValueError), (dict(mode="dynamic", s_max=float("nan")), ValueError),
                     (dict(mode="static", range=0.0), ValueError), (dict(mode="static", range=float("inf")), ValueError),
                     (dict(mode="median"), ValueError)):
        with pytest.raises(exc):
            ctx.threshold_step(x, m, z, h.clone(), _thr(**bad), *([1.0] * 6), 1)
    with pytest.raises(NotImplementedError):      # 4 x 65 x 65 > 16384 elements: DD_ERR_UNSUPPORTED
        big = torch.zeros(1, 4, 65, 65, device="cuda")
        ctx.threshold_step(big, big.clone(), None, big.clone(), thr, *([1.0] * 6), 0)
    thr_p = L.dd_x0_threshold(7, 0.5, 1.0, 1.0)
    assert ctx.lib.dd_threshold_step(ctx.handle, x.data_ptr(), m.data_ptr(), None, h.data_ptr(), C.byref(thr_p), *([1.0] * 6), 0, x.data_ptr(),
                                     B, C_, S, None) == L.DD_ERR_INVALID and "mode" in ctx.lib.dd_last_error(ctx.handle).decode()
    assert ctx.lib.dd_threshold_step(ctx.handle, x.data_ptr(), m.data_ptr(), None, h.data_ptr(), None, *([1.0] * 6), 0, x.data_ptr(),
                                     B, C_, S, None) == L.DD_ERR_INVALID


# ---- GPU: the loop ----------------------------------------------------------------------------------------------------------------
def _model(S=8, cond=False, precision="bf16", depth=3, seed=42, max_batch=12):
    return tiny_model(max_batch, seed, precision, img_size=S, depth=depth, **(dict(num_classes=11) if cond else {}))


def _plan(sampler_kind, par="predict_noise"):
    from duodiff_amd import sampler
    kw = {"ode": dict(solver="dpmsolver++", solver_steps=6), "sde": dict(solver="sde-dpmsolver++", solver_steps=6),
          "ddim": dict(use_ddim=True, ddim_steps=7, ddim_eta=0.02), "ddpm": dict(num_steps=12)}[sampler_kind]
    return sampler.step_plan(par, threshold=_thr("static"), **kw)


def _known(B, S, seed=3):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(B, 3, S, S, generator=g).clamp(-1, 1).cuda()
    mask = torch.tensor([0.0, 1.0, 0.25])[torch.randint(0, 3, (B, 1, S, S), generator=g)].cuda()
    return x0, mask


THR = {"dynamic": dict(quantile=0.995), "static": dict(range=1.0)}


@gpu
@pytest.mark.parametrize("mods", ["plain", "cfg", "autoguided", "known"])
@pytest.mark.parametrize("kind,S,prec,mode", [("ode", 8, "fp32", "dynamic"), ("sde", 16, "bf16", "dynamic"), ("ddim", 8, "bf16", "static"),
                                              ("ddpm", 16, "fp32", "dynamic"), ("sde", 8, "bf16", "static")])
def test_loop_equals_the_composition_of_its_parts(kind, S, prec, mode, mods):
    """graph, eager, and two chains forced at B = 6, all against dd_forward* + dd_threshold_step + dd_known_blend, bit for bit (x and h)"""
    from duodiff_amd.engine import Autoguidance
    B = 6
    em = _model(S, cond=mods == "cfg", precision=prec)
    kw = {}
    if mods == "cfg":
        kw = dict(guidance=(1.7, NULL), y=labels(B, 10, 4))
    elif mods == "autoguided":
        kw = dict(guidance=Autoguidance(_model(S, precision=prec, depth=1, seed=41), 1.3))
    elif mods == "known":
        kw = dict(region=_known(B, S))
    plan, thr, st = _plan(kind), _thr(mode, **THR[mode]), side_stream()
    x_in = images(B, 3, S, 2)
    xc, hc = run_steps("threshold", em, x_in, plan, st, threshold=thr, **kw)
    assert torch.isfinite(xc).all() and not torch.equal(xc, x_in)
    for name, args in (("graph", dict(flags=L.DD_DEV_NO_CHAINS)), ("eager", dict(use_graph=False)), ("two chains", dict(flags=L.DD_DEV_FORCE_CHAINS))):
        x, h, chains = run_loop("threshold", em, x_in, plan, st, threshold=thr, **kw, **args)
        assert chains == (2 if name == "two chains" else 1), (name, chains)
        assert torch.equal(x, xc) and torch.equal(h, hc), f"{name}: the loop differs from the composition"
    plain, _, _ = run_loop("multistep", em, x_in, plan, st, **kw)
    assert not torch.equal(plain, xc), "thresholding changed nothing: the test does not exercise it"


@gpu
@pytest.mark.parametrize("kind", ["sde", "ddpm"])
def test_cut_loop_resumes_to_the_bits_of_the_uncut_loop(kind):
    B, S = 6, 8
    em, st = _model(S), side_stream()
    plan, thr, x_in = _plan(kind), _thr("dynamic", quantile=0.995), images(B, 3, S, 2)
    n = len(plan.rows["t"])
    whole = run_loop("threshold", em, x_in, plan, st, threshold=thr, flags=L.DD_DEV_FORCE_CHAINS, region=_known(B, S))
    cut = run_loop("threshold", em, x_in, plan, st, threshold=thr, flags=L.DD_DEV_FORCE_CHAINS, region=_known(B, S), cuts=(1, n // 2))
    assert torch.equal(whole[0], cut[0]) and torch.equal(whole[1], cut[1])


@gpu
def test_graph_keys_separate_thresholded_and_plain_calls():
    """alternating calls on one model reproduce each one's stand-alone bits; a following dd_sample is untouched; range = 3e38 is the plain
    loop's first step within 4 ulp"""
    from duodiff_amd import sampler
    from duodiff_amd.engine import sample_loop
    B, S = 6, 8
    em, st = _model(S), side_stream()
    plan, x_in = _plan("sde"), images(B, 3, S, 2)
    variants = [None, _thr("dynamic", quantile=0.995), _thr("dynamic", quantile=0.9), _thr("dynamic", quantile=0.995, s_max=2.0),
                _thr("static", range=1.0), _thr("static", range=0.5)]
    alone = []
    for thr in variants:
        fresh = _model(S)
        alone.append(run_loop("threshold", fresh, x_in, plan, side_stream(), threshold=thr)[0])
        del fresh
    assert len({a.cpu().numpy().tobytes() for a in alone}) == len(variants)

    def ddpm(model):
        x = x_in.clone()
        with torch.cuda.stream(st):
            sample_loop(model.ctx, model, None, x, t_start=999, t_end=994, seed=9, stream=st)
        st.synchronize()
        return x
    before = ddpm(em)
    for _ in range(2):
        for thr, want in zip(variants, alone):
            assert torch.equal(run_loop("threshold", em, x_in, plan, st, threshold=thr)[0], want), thr
    assert torch.equal(ddpm(em), before), "a thresholded call changed a following dd_sample"
    # one step, nothing clipped: unfolded rows through the thresholded loop vs the folded plain loop
    ode = _plan("ode")
    one = sampler.StepPlan("multistep", {k: v[:1] for k, v in ode.rows.items()}, [False], None, ode.lands[:1])
    folded = sampler.step_plan("predict_noise", solver="dpmsolver++", solver_steps=6)
    fold1 = sampler.StepPlan("multistep", {k: v[:1] for k, v in folded.rows.items()}, [False], None, folded.lands[:1])
    got = run_loop("threshold", em, x_in, one, st, threshold=_thr("static", range=3e38))[0].cpu().numpy()
    ref = run_loop("multistep", em, x_in, fold1, st)[0].cpu().numpy()
    eps = torch.empty_like(x_in)
    em.forward(x_in, float(ode.rows["t"][0]), None, out=eps)
    torch.cuda.synchronize()
    mag = np.abs(fold1.rows["a"][0] * x_in.cpu().numpy()) + np.abs(fold1.rows["b"][0] * eps.cpu().numpy())
    ulps = np.abs(got.astype(np.float64) - ref) / np.spacing(mag)
    print(f"range 3e38 vs the plain loop's first step: worst {ulps.max():.2f} ulp")
    assert np.isfinite(got).all() and ulps.max() <= 4.0


@gpu
def test_invalid_threshold_calls_are_rejected_before_anything_is_enqueued():
    from duodiff_amd.engine import Model
    B = 4
    em = _model(8, max_batch=B)
    ctx, lib = em.ctx, em.ctx.lib
    ee = Model(ctx, ModelParams.from_dict(dict(TINY, depth=3)), B)
    ee.enable_early_exit("mlp_probe_per_layer")
    rows = _plan("ode").rows
    keep = {k: np.ascontiguousarray(rows[k], F) for k in "tabcdpq"}
    keep.update({k: np.ascontiguousarray(rows[k], np.int32) for k in ("noise", "hist")})
    st = side_stream()
    n0 = lib.dd_dev_graph_captures(ctx.handle)
    ok = (L.DD_X0_DYNAMIC, 0.995, 1.0, float("inf"))
    cases = [("null", None, "dd_x0_threshold"), ("mode", (5, 0.5, 1.0, 1.0), "mode"), ("q0", (1, 0.0, 1.0, 1.0), "quantile"),
             ("q2", (1, 1.5, 1.0, 1.0), "quantile"), ("r0", (0, 0.5, 0.0, 1.0), "range"), ("rinf", (0, 0.5, float("inf"), 1.0), "range"),
             ("smax", (1, 0.5, 1.0, 0.5), "s_max"), ("snan", (1, 0.5, 1.0, float("nan")), "s_max"), ("host_noise", ok, "noise"),
             ("early_exit", ok, "early-exit"), ("h_dev", ok, "h_dev"), ("both", ok, "exclusive")]
    for what, t, msg in cases:
        model = ee if what == "early_exit" else em
        x0 = images(B, 3, 8, 2)
        x, h = x0.clone(), torch.zeros_like(x0)
        a = L.dd_multistep_sample_args()
        a.first, a.late, a.n_steps, a.switch_after = model.handle, None, 3, 3
        for k in "tabcdpq":
            setattr(a, k, keep[k].ctypes.data_as(C.POINTER(C.c_float)))
        a.noise, a.hist = (keep[k].ctypes.data_as(C.POINTER(C.c_int32)) for k in ("noise", "hist"))
        a.noise_mode = L.DD_NOISE_BUFFER if what == "host_noise" else L.DD_NOISE_PHILOX
        a.use_graph, a.seed, a.y_dev, a.x_dev, a.B = 1, 1, None, x.data_ptr(), B
        a.h_dev = None if what == "h_dev" else h.data_ptr()
        thr = None if t is None else C.byref(L.dd_x0_threshold(*t))
        g = C.byref(L.dd_guidance(1.0, 0)) if what == "both" else None
        ag = C.byref(L.dd_autoguidance(em.handle, 1.0)) if what == "both" else None
        with torch.cuda.stream(st):
            rc = lib.dd_sample_multistep_threshold(ctx.handle, C.byref(a), g, ag, None, thr, C.c_void_p(st.cuda_stream))
        st.synchronize()
        err = lib.dd_last_error(ctx.handle).decode()
        assert rc == L.DD_ERR_INVALID and msg in err, (what, rc, err)
        assert torch.equal(x, x0) and not h.any(), f"{what}: something was enqueued"
    assert lib.dd_dev_graph_captures(ctx.handle) == n0


# ---- GPU: numerics and hygiene ---------------------------------------------------------------------------------------------------
NUM_SEED, NUM_START, NUM_QT = 61, 12, 0.995


def _float64_reference(B=3):
    """6 thresholded DPM-Solver++(2M) steps in float64 on the numpy oracle; also the smallest relative gap between the quantile pair
    v[i], v[i + 1] and their neighbours over every step and image (a swap there would move s by more than rounding)"""
    import oracle
    from duodiff_amd import sampler
    mp = ModelParams.from_dict(dict(TINY))
    sd = synthetic_state_dict(mp, NUM_SEED)
    orc = oracle.UViTOracle(mp.as_dict(), {k: v.numpy() for k, v in sd.items()})
    x0 = torch.randn(B, 3, 8, 8, generator=torch.Generator().manual_seed(NUM_START))
    ts = sampler.multistep_grid(6)
    ab = _tables64()["alphas_bar"]
    r = sampler.multistep_rows("dpmsolver++", ab[ts], 2, unfolded=True)
    thr = _thr("dynamic", quantile=NUM_QT)
    x, h, gap = x0.numpy().astype(np.float64), np.zeros((B, 3, 8, 8)), np.inf
    for k in range(6):
        m = orc(x.astype(F), np.full((B,), float(ts[k]), F)).astype(np.float64)
        pred = r["p"][k] * x + r["q"][k] * m
        for b in range(B):
            v = np.sort(np.abs(pred[b]).ravel())
            i = int(np.floor(np.float64(F(NUM_QT)) * (v.size - 1)))
            for lo in (i - 1, i + 1):
                if 0 <= lo and lo + 1 < v.size:
                    gap = min(gap, (v[lo + 1] - v[lo]) / v[lo + 1])
        x, h = _restate(x, m, None, h, thr, *(r[c][k] for c in "abcdpq"), r["hist"][k], dtype=np.float64)
    return x0, ts, x, gap


def test_float64_reference_has_no_near_ties_at_its_quantiles():
    _, _, x, gap = _float64_reference()
    print(f"float64 thresholded solver on the oracle: smallest relative gap around a quantile pair {gap:.3e}, |x| max {np.abs(x).max():.3f}")
    assert np.isfinite(x).all() and gap > 1e-3


@gpu
def test_fp32_engine_matches_the_float64_thresholded_solver_on_the_oracle():
    """6 thresholded DPM-Solver++ steps, dynamic, quantile 0.995: the fp32 engine against the float64 restatement on the numpy oracle,
    max abs <= 2e-3 -- the bound of tests/test_multistep.py's unthresholded twin (1e-3) times the Lipschitz constant 2 of x0 -> xh."""
    from duodiff_amd import sampler
    from duodiff_amd.engine import sample_multistep_threshold_loop
    B = 3
    x0, ts, x, gap = _float64_reference(B)
    assert gap > 1e-3
    m32, _ = uvit(dict(TINY), NUM_SEED, "fp32", B)
    em = m32.engine_model(B)
    xd, hd = x0.cuda(), torch.zeros(B, 3, 8, 8, device="cuda")
    sample_multistep_threshold_loop(em.ctx, em, None, xd, hd, sampler.multistep_coefficients("dpmsolver++", ts, 2, unfolded=True),
                                    _thr("dynamic", quantile=NUM_QT), noise="none")
    torch.cuda.synchronize()
    err = float(np.abs(xd.cpu().numpy() - x).max())
    print(f"fp32 engine vs float64 thresholded solver on the oracle, 6 steps: max abs {err:.3e} (|x| max {np.abs(x).max():.3f})")
    assert np.isfinite(err) and err <= 2e-3


@gpu
def test_no_kernel_of_a_thresholded_call_depends_on_stale_bytes():
    """Both chains' workspaces and the context's model-output scratch are filled with NaN bytes on the launch stream before a model's
    first thresholded call (h NaN-filled too: step 0 has no history); the samples equal those of a fresh model, bit for bit."""
    B, S = 6, 8
    plan, thr, x_in, st = _plan("sde"), _thr("dynamic", quantile=0.995), images(B, 3, S, 2), side_stream()
    outs = []
    for poison in (False, True):
        em = _model(S, cond=True, seed=73)
        y = labels(B, 10, 15)
        h0 = None
        if poison:
            em.ctx.check(em.ctx.lib.dd_dev_poison_workspaces(em.ctx.handle, em.handle, st.cuda_stream))
            h0 = torch.full_like(x_in, float("nan"))
        outs.append(run_loop("threshold", em, x_in, plan, st, threshold=thr, flags=L.DD_DEV_FORCE_CHAINS, guidance=(1.5, NULL), y=y, region=_known(B, S), h0=h0))
        del em
    assert outs[0][2] == outs[1][2] == 2
    assert torch.isfinite(outs[0][0]).all() and torch.isfinite(outs[1][1]).all()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "poisoned run differs"
