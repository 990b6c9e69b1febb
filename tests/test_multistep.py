"""DPM-Solver++ multistep sampling (Lu et al., 2022): the host rows (sampler.multistep_coefficients / multistep_rows), the history
register fused into the step's last kernel (dd_sample_multistep[_guided]), the elementwise row (dd_multistep_step) and the
--dpm_solver options.

CPU tests: the rows against DDIM and against a textbook solver, the order of convergence on Gaussian data, the command line and the
binding.  GPU tests (marked): the kernels against a float32 emulation, the loop forms, chains, cuts, guidance, graph keys, stale bytes
and the fp32 engine against the numpy oracle, bit for bit where the arithmetic is the same.
"""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, TINY
from duodiff_amd import _lib as L
from duodiff_amd.config import ModelParams
from duodiff_amd.weights import synthetic_state_dict
from loop_support import NULL, celeba_pair, cli_argv, dev_flags, engine_pair, images, labels, run_loop, run_steps, side_stream, uvit

gpu = pytest.mark.gpu
CELEBA = REPO / "configs" / "uvit_celeba.yaml"


def _abar():
    from duodiff_amd.engine import schedule_tables
    return schedule_tables()["alphas_bar"].astype(np.float64)


# ---- CPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [10, 20, 25, 50, 100, 999])
def test_order1_ode_rows_equal_ddim(n):
    """Order-1 DPM-Solver++ is DDIM with eta = 0 in exact arithmetic: a within 2 ulp, b within 1e-4 relative (DDIM's own fp32
    formula for b cancels), no history, no noise."""
    from duodiff_amd import sampler
    ts = sampler.multistep_grid(n)
    r = sampler.multistep_coefficients("dpmsolver++", ts, order=1)
    assert r["a"].dtype == np.float32 and len(r["t"]) == n and list(r["t"]) == [float(t) for t in ts[:-1]]
    assert not r["hist"].any() and not r["noise"].any() and not r["d"].any()
    for k, (t, s) in enumerate(zip(ts[:-1], ts[1:])):
        a, b, _ = sampler.affine_coefficients("ddim", int(t), int(s), 0.0)
        ulp = np.spacing(np.float32(a))
        assert abs(float(r["a"][k]) - float(a)) <= 2 * ulp, (t, s, r["a"][k], a)
        assert abs(float(r["b"][k]) - float(b)) <= 1e-4 * abs(float(b)), (t, s, r["b"][k], b)


def _textbook(kind, ab, x, eps_fn, zs, order=2):
    """DPM-Solver++(2M) / SDE-DPM-Solver++(2M) (midpoint) written directly in x0 form, float64, first-order first and last steps"""
    alpha, sigma = np.sqrt(ab), np.sqrt(1 - ab)
    lam = np.log(alpha / sigma)
    n = len(ab) - 1
    x0_prev, h_prev = None, None
    for k in range(n):
        x0 = (x - sigma[k] * eps_fn(x, k)) / alpha[k]
        h = lam[k + 1] - lam[k]
        if order == 1 or k == 0 or k == n - 1:
            D = x0
        else:
            r = h_prev / h
            D = x0 + (x0 - x0_prev) / (2 * r)
        if kind == "dpmsolver++":
            x = sigma[k + 1] / sigma[k] * x - alpha[k + 1] * (np.exp(-h) - 1) * D
        else:
            x = (sigma[k + 1] / sigma[k] * np.exp(-h) * x + alpha[k + 1] * (1 - np.exp(-2 * h)) * D
                 + sigma[k + 1] * np.sqrt(1 - np.exp(-2 * h)) * zs[k])
        x0_prev, h_prev = x0, h
    return x


def _apply_rows(r, x, eps_fn, zs):
    h = np.full_like(x, np.nan)
    for k in range(len(r["a"])):
        m = eps_fn(x, k)
        v = r["a"][k] * x + r["b"][k] * m
        if r["hist"][k]:
            v = v + r["d"][k] * h
        if r["noise"][k]:
            v = v + r["c"][k] * zs[k]
        h = r["p"][k] * x + r["q"][k] * m
        x = v
    return x


@pytest.mark.parametrize("kind", ["dpmsolver++", "sde-dpmsolver++"])
@pytest.mark.parametrize("order", [1, 2])
def test_rows_match_a_textbook_solver(kind, order):
    """The float64 rows, applied as the kernel applies them, equal a textbook DPM-Solver++ in x0 form to 1e-12 relative (a nonlinear
    stand-in model, fixed z)."""
    from duodiff_amd import sampler
    ts = sampler.multistep_grid(20)
    ab = _abar()[ts]
    rng = np.random.default_rng(3)
    x = rng.standard_normal(64)
    zs = rng.standard_normal((20, 64))
    eps_fn = lambda v, k: np.tanh(0.7 * v + 0.01 * k) + 0.1 * v
    r = sampler.multistep_rows(kind, ab, order)
    got, want = _apply_rows(r, x, eps_fn, zs), _textbook(kind, ab, x, eps_fn, zs, order)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_predict_original_rows():
    """predict_original: x0 = m, i.e. (p, q) = (0, 1); the same solver as predict_noise fed m = (x - sigma eps) / alpha."""
    from duodiff_amd import sampler
    ts = sampler.multistep_grid(15)
    ab = _abar()[ts]
    alpha, sigma = np.sqrt(ab), np.sqrt(1 - ab)
    eps_fn = lambda v, k: np.sin(v) + 0.3 * v
    x = np.linspace(-2, 2, 33)
    zs = np.zeros((15, 33))
    ro = sampler.multistep_rows("dpmsolver++", ab, 2, "predict_original")
    assert (ro["p"] == 0).all() and (ro["q"] == 1).all()
    got = _apply_rows(ro, x, lambda v, k: (v - sigma[k] * eps_fn(v, k)) / alpha[k], zs)
    want = _apply_rows(sampler.multistep_rows("dpmsolver++", ab, 2, "predict_noise"), x, eps_fn, zs)
    assert np.abs(got - want).max() <= 1e-11


def _gauss_error(ab, s2, order, lower_order_final):
    """|x_final - exact| of the probability-flow ODE on N(0, s2 I) data from x = 1 (exact eps: sigma x / (alpha^2 s2 + sigma^2))"""
    from duodiff_amd import sampler
    alpha, sigma = np.sqrt(ab), np.sqrt(1 - ab)
    r = sampler.multistep_rows("dpmsolver++", ab, order, lower_order_final=lower_order_final)
    x = _apply_rows(r, 1.0, lambda v, k: sigma[k] * v / (alpha[k] ** 2 * s2 + sigma[k] ** 2), None)
    exact = np.sqrt(alpha[-1] ** 2 * s2 + sigma[-1] ** 2) / np.sqrt(alpha[0] ** 2 * s2 + sigma[0] ** 2)
    return abs(x - exact)


@pytest.mark.parametrize("s2", [0.05, 1.0])
def test_order_of_convergence_on_gaussian_data(s2):
    """A continuous grid (log abar interpolated linearly, t 999 -> 100), only step 0 first order: each doubling of N cuts order 2's
    error by >= 3x and order 1's by 1.8 - 2.2x."""
    log_ab = np.log(_abar())

    def grid(n):
        return np.exp(np.interp(np.linspace(999, 100, n + 1), np.arange(1000), log_ab))
    for order in (1, 2):
        e = [_gauss_error(grid(n), s2, order, False) for n in (20, 40, 80)]
        ratios = [e[0] / e[1], e[1] / e[2]]
        print(f"s2 {s2} order {order}: errors {e} ratios {ratios}")
        for q in ratios:
            assert (q >= 3.0) if order == 2 else (1.8 <= q <= 2.2), (order, ratios)


@pytest.mark.parametrize("n", [15, 20, 25, 40])
@pytest.mark.parametrize("s2", [0.05, 0.25, 1.0])
def test_second_order_beats_first_on_the_product_grid(n, s2):
    """The integer grid to t = 0 with the first-order last step: order 2's final error is below order 1's."""
    from duodiff_amd import sampler
    ab = _abar()[sampler.multistep_grid(n)]
    assert _gauss_error(ab, s2, 2, True) < _gauss_error(ab, s2, 1, True)


def test_rows_grid_and_flags():
    from duodiff_amd import sampler
    ts = sampler.multistep_grid(20)
    assert ts[0] == 999 and ts[-1] == 0 and len(ts) == 21
    r = sampler.multistep_coefficients("sde-dpmsolver++", ts, 2)
    assert list(r["hist"]) == [0] + [1] * 18 + [0]
    assert list(r["noise"]) == [1] * 19 + [0]          # no z on the step landing on t = 0
    assert r["c"][0] > 0 and np.isfinite([r[k] for k in "abcdpq"]).all()
    assert sampler.multistep_coefficients("dpmsolver++", sampler.multistep_grid(1), 2)["hist"].tolist() == [0]
    for bad in (0, 1000, -3):
        with pytest.raises(ValueError):
            sampler.multistep_grid(bad)
    with pytest.raises(ValueError, match="predict_previous"):
        sampler.multistep_coefficients("dpmsolver++", ts, 2, "predict_previous")
    with pytest.raises(ValueError):
        sampler.multistep_coefficients("unipc", ts, 2)


def _argv(*extra):
    return cli_argv(CELEBA, *extra)


def test_cli_solver_options_and_defaults():
    from duodiff_amd import sampler
    a = sampler.get_args(_argv())
    assert a.dpm_solver is None and a.dpm_solver_steps == 20 and a.dpm_solver_order == 2 and not a.use_ddim
    assert sampler.solver_kwargs(a) == dict(solver=None, solver_steps=20, solver_order=2)
    a = sampler.get_args(_argv("--dpm_solver", "sde", "--dpm_solver_steps", "15", "--dpm_solver_order", "1"))
    assert sampler.solver_kwargs(a) == dict(solver="sde-dpmsolver++", solver_steps=15, solver_order=1)
    assert sampler.solver_kwargs(sampler.get_args(_argv("--dpm_solver", "ode")))["solver"] == "dpmsolver++"
    with pytest.raises(SystemExit):
        sampler.get_args(_argv("--dpm_solver", "ode", "--dpm_solver_order", "3"))


@pytest.mark.parametrize("entry", ["sampler", "dist"])
@pytest.mark.parametrize("extra,match", [
    (["--dpm_solver", "ode", "--use_ddim"], "exclusive"),
    (["--dpm_solver", "sde", "--parametrization", "predict_previous"], "predict_previous"),
    (["--dpm_solver", "ode", "--dpm_solver_steps", "0"], "outside"),
    (["--dpm_solver", "ode", "--dpm_solver_steps", "1000"], "outside"),
])
def test_cli_rejects_invalid_solver_options_before_any_gpu_work(tmp_path, entry, extra, match):
    from duodiff_amd import dist, sampler
    argv = _argv(*extra)
    argv[argv.index("--output_folder") + 1] = str(tmp_path / "out")
    with pytest.raises(ValueError, match=match):
        (sampler.main if entry == "sampler" else dist.main)(argv)


def test_lib_binds_the_multistep_entry_points():
    assert L.ABI_VERSION == 6
    # dd_affine_sample_args' fields (104 bytes with the tail padding), then d, p, q, hist, h_dev
    assert C.sizeof(L.dd_affine_sample_args) == 104 and C.sizeof(L.dd_multistep_sample_args) == 144
    assert L.dd_multistep_sample_args.d.offset == 104 and L.dd_multistep_sample_args.h_dev.offset == 136
    assert L.SIGNATURES["dd_sample_multistep"][1] == [C.c_void_p, C.POINTER(L.dd_multistep_sample_args), C.c_void_p]
    assert L.SIGNATURES["dd_sample_multistep_guided"][1] == [C.c_void_p, C.POINTER(L.dd_multistep_sample_args),
                                                             C.POINTER(L.dd_guidance), C.c_void_p]
    assert len(L.SIGNATURES["dd_multistep_step"][1]) == 15
    lib = L.load()
    assert lib.dd_abi_version() == 6
    for name in ("dd_multistep_step", "dd_sample_multistep", "dd_sample_multistep_guided"):
        assert hasattr(lib, name)


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def _tiny_pair(max_batch, seeds=(41, 42), **kw):
    return engine_pair(dict(TINY, depth=1, **kw), dict(TINY, depth=3, **kw), seeds, max_batch)


@pytest.fixture(scope="module", name="celeba_pair")
def _celeba_pair_of_the_module():
    return celeba_pair(32)


def _rows(kind="sde-dpmsolver++", n=20, order=2, steps=None):
    from duodiff_amd import sampler
    r = sampler.multistep_coefficients(kind, sampler.multistep_grid(n), order)
    return r if steps is None else {k: v[:steps] for k, v in r.items()}


def _loop(es, ef, x0, rows, stream, **kw):
    """the device loop from x0 on the pair; kw: run_loop's -> (x, h, chains of the last call)"""
    return run_loop("multistep", es, x0, rows, stream, late=ef, **kw)


def _host_loop(es, ef, x0, rows, stream, **kw):
    """step by step: dd_forward[_guided] + dd_multistep_step, z as the device loop draws it"""
    return run_steps("multistep", es, x0, rows, stream, late=ef, **kw)


@gpu
def test_multistep_step_kernel_bit_exact():
    """dd_multistep_step == a numpy float32 emulation of the rounding order (products rounded, added left to right); with
    use_hist = 0 a NaN-filled h is not read."""
    from duodiff_amd.engine import Context
    ctx = Context.get()
    g = torch.Generator().manual_seed(1)
    n = 3 * 1000 + 17
    x, m, z, h = (torch.randn(n, generator=g) for _ in range(4))
    co = [np.float32(v) for v in (0.9813, -0.2371, 0.0417, -0.5333, 1.0734, -0.6127)]
    a, b, c, d, p, q = co
    xn, mn, zn, hn = (v.numpy() for v in (x, m, z, h))
    for use_hist in (1, 0):
        for with_z in (True, False):
            hd = h.cuda() if use_hist else torch.full((n,), float("nan"), device="cuda")
            out = ctx.multistep_step(x.cuda(), m.cuda(), z.cuda() if with_z else None, hd, *co, use_hist)
            torch.cuda.synchronize()
            want = a * xn + b * mn
            if use_hist:
                want = want + d * hn
            if with_z:
                want = want + c * zn
            assert want.dtype == np.float32
            assert np.isfinite(out.cpu().numpy()).all()
            assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32)), (use_hist, with_z)
            assert np.array_equal(hd.cpu().numpy().view(np.uint32), (p * xn + q * mn).view(np.uint32))
    xi = x.cuda()      # in place (out aliases x)
    hd = h.cuda()
    ctx.multistep_step(xi, m.cuda(), None, hd, *co, 1, out=xi)
    torch.cuda.synchronize()
    assert np.array_equal(xi.cpu().numpy(), a * xn + b * mn + d * hn)
    with pytest.raises(ValueError):
        ctx.multistep_step(xi, m.cuda(), None, xi, *co, 1)          # h aliasing x


@gpu
@pytest.mark.parametrize("kind", ["dpmsolver++", "sde-dpmsolver++"])
def test_loop_forms_agree(kind):
    """TINY pair, backbone switch inside: graph replay == eager launches == dd_forward + dd_multistep_step, bit for bit (x and h)."""
    B = 4
    es, ef, _ = _tiny_pair(max_batch=B)
    x0 = images(B, 3, 8, 2)
    rows = _rows(kind, n=10)
    st = side_stream()
    xg, hg, _ = _loop(es, ef, x0, rows, st, switch_after=4, use_graph=True)
    xe, he, _ = _loop(es, ef, x0, rows, st, switch_after=4, use_graph=False)
    xm, hm = _host_loop(es, ef, x0, rows, st, switch_after=4)
    assert torch.isfinite(xg).all() and not torch.equal(xg, x0)
    assert torch.equal(xg, xe) and torch.equal(hg, he), "graph replay differs from eager launches"
    assert torch.equal(xg, xm) and torch.equal(hg, hm), "device loop differs from forward + multistep_step"


@gpu
@pytest.mark.parametrize("case", ["tiny_forced", "celeba_default"])
def test_two_chains_equal_one_chain(case, request):
    if case == "tiny_forced":
        B, S, force = 6, 8, L.DD_DEV_FORCE_CHAINS
        es, ef, _ = _tiny_pair(max_batch=B)
    else:
        B, S, force = 32, 64, 0
        es, ef, _ = request.getfixturevalue("celeba_pair")
    x0 = images(B, 3, S, 3)
    rows = _rows("sde-dpmsolver++", n=20, steps=8)
    st = side_stream()
    x2, h2, c2 = _loop(es, ef, x0, rows, st, switch_after=5, flags=force)
    x1, h1, c1 = _loop(es, ef, x0, rows, st, switch_after=5, flags=L.DD_DEV_NO_CHAINS)
    assert (c2, c1) == (2, 1)
    assert torch.isfinite(x1).all() and not torch.equal(x1, x0)
    assert torch.equal(x2, x1) and torch.equal(h2, h1), "two chains differ from one"


@gpu
@pytest.mark.parametrize("case", ["tiny_forced", "celeba_default"])
def test_cut_loop_equals_the_uncut_loop(case, request):
    """A loop cut into calls (h and the Philox counter carried across) == one call, bit for bit; get_samples' cut path too."""
    if case == "tiny_forced":
        B, S, force = 6, 8, L.DD_DEV_FORCE_CHAINS
        es, ef, _ = _tiny_pair(max_batch=B)
    else:
        B, S, force = 32, 64, 0
        es, ef, _ = request.getfixturevalue("celeba_pair")
    x0 = images(B, 3, S, 4)
    rows = _rows("sde-dpmsolver++", n=12)
    st = side_stream()
    xu, hu, _ = _loop(es, ef, x0, rows, st, switch_after=6, flags=force)
    xc, hc, _ = _loop(es, ef, x0, rows, st, switch_after=6, flags=force, cuts=(3, 6, 7))
    assert torch.isfinite(xu).all() and torch.equal(xu, xc) and torch.equal(hu, hc), "a cut loop differs from the uncut loop"


@gpu
@pytest.mark.parametrize("S", [8, 16])
def test_guided_multistep(S):
    """Class-conditional TINY pair (S = 8: one tile of 64 live lanes, S = 16: a full tile), chains forced: scale 0 == the unguided loop with the
    same labels (SDE, Philox noise); scale 0.4 ODE == forward_guided + multistep_step, bit for bit."""
    B = 6
    es, ef, _ = _tiny_pair(max_batch=2 * B, num_classes=11, img_size=S)
    x0 = images(B, 3, S, 5)
    y = labels(B, NULL, 6)
    st = side_stream()
    rows = _rows("sde-dpmsolver++", n=10)
    xu, hu, cu = _loop(es, ef, x0, rows, st, switch_after=3, y=y, flags=L.DD_DEV_FORCE_CHAINS)
    x0g, h0g, cg = _loop(es, ef, x0, rows, st, switch_after=3, y=y, guidance=(0.0, NULL), flags=L.DD_DEV_FORCE_CHAINS)
    assert cu == cg == 2
    assert torch.isfinite(xu).all() and torch.equal(xu, x0g) and torch.equal(hu, h0g), "guided scale 0 differs from the unguided loop"
    rows = _rows("dpmsolver++", n=8)
    xg, hg, _ = _loop(es, ef, x0, rows, st, switch_after=3, y=y, guidance=(0.4, NULL), flags=L.DD_DEV_FORCE_CHAINS)
    xm, hm = _host_loop(es, ef, x0, rows, st, switch_after=3, y=y, guidance=(0.4, NULL))
    assert not torch.equal(xg, x0g)
    assert torch.equal(xg, xm) and torch.equal(hg, hm), "guided loop differs from forward_guided + multistep_step"


@gpu
@pytest.mark.parametrize("case", ["tiny_forced", "celeba_default"])
def test_ddim_rows_reproduce_the_affine_loop(case, request):
    """The multistep loop fed affine rows (d = p = q = 0, no history) == dd_sample_affine bit for bit: the affine arithmetic is
    untouched by the history term.  DDIM's rows (eta 0, no noise) and predict_original's (Philox z on every step)."""
    from duodiff_amd import sampler
    from duodiff_amd.engine import sample_affine_loop
    if case == "tiny_forced":
        B, S, force = 6, 8, L.DD_DEV_FORCE_CHAINS
        es, ef, _ = _tiny_pair(max_batch=B)
    else:
        B, S, force = 32, 64, 0
        es, ef, _ = request.getfixturevalue("celeba_pair")
    x0 = images(B, 3, S, 7)
    ts = np.linspace(0, 999, 11).astype(int)[::-1]
    pairs = [(int(t), int(s)) for t, s in zip(ts[:-1], ts[1:])]
    tables = {"ddim": ([float(t) for t, _ in pairs], [sampler.affine_coefficients("ddim", t, s, 0.0) for t, s in pairs], [0] * 10),
              "predict_original": ([float(t) for t in range(999, 989, -1)],
                                   [sampler.affine_coefficients("predict_original", t) for t in range(999, 989, -1)], [1] * 10)}
    st = side_stream()
    for name, (t, co, nz) in tables.items():
        n = len(t)
        rows = dict(t=t, a=[c[0] for c in co], b=[c[1] for c in co], c=[c[2] for c in co], noise=nz, d=np.zeros(n), p=np.zeros(n),
                    q=np.zeros(n), hist=np.zeros(n, np.int32))
        xm, hm, _ = _loop(es, ef, x0, rows, st, switch_after=4, flags=force, seed=8)
        xa = x0.clone()
        with dev_flags(es.ctx, force), torch.cuda.stream(st):
            sample_affine_loop(es.ctx, es, ef, xa, rows["t"], rows["a"], rows["b"], rows["c"], rows["noise"], switch_after=4, seed=8,
                               noise="philox", stream=st)
            st.synchronize()
        assert torch.isfinite(xa).all() and not torch.equal(xa, x0), name
        assert torch.equal(xm, xa), f"multistep loop with {name} rows differs from dd_sample_affine"
        assert not hm.any()


@gpu
def test_affine_and_multistep_calls_do_not_share_graphs():
    """Affine, multistep, affine, multistep on one model pair: each call reproduces its own kind's first result, the second round
    captures no graph (each kind keeps its own), and a fresh pair gives the same multistep result."""
    from duodiff_amd import sampler
    from duodiff_amd.engine import sample_affine_loop
    B = 4
    x0 = images(B, 3, 8, 9)
    rows = _rows("dpmsolver++", n=10)
    co = [sampler.affine_coefficients("ddim", int(t), int(s), 0.0)
          for t, s in zip(sampler.multistep_grid(10)[:-1], sampler.multistep_grid(10)[1:])]
    st = side_stream()

    def affine(es, ef):
        x = x0.clone()
        with torch.cuda.stream(st):
            sample_affine_loop(es.ctx, es, ef, x, rows["t"], [c[0] for c in co], [c[1] for c in co], [c[2] for c in co],
                               [0] * 10, switch_after=4, seed=1, noise="philox", stream=st)
        st.synchronize()
        return x

    es, ef, _ = _tiny_pair(max_batch=B)
    lib, h = es.ctx.lib, es.ctx.handle
    a1 = affine(es, ef)
    m1 = _loop(es, ef, x0, rows, st, switch_after=4)[0]
    n0 = lib.dd_dev_graph_captures(h)
    a2 = affine(es, ef)
    m2 = _loop(es, ef, x0, rows, st, switch_after=4)[0]
    assert lib.dd_dev_graph_captures(h) == n0, "the second round re-captured a graph"
    fs, ff, _ = _tiny_pair(max_batch=B)
    m_fresh = _loop(fs, ff, x0, rows, st, switch_after=4)[0]
    assert not torch.equal(a1, m1)
    assert torch.equal(a1, a2), "affine call replayed a stale graph"
    assert torch.equal(m1, m2) and torch.equal(m1, m_fresh), "multistep call replayed a stale graph"


@gpu
def test_poisoned_workspaces_and_history():
    """Both chains' workspaces NaN-poisoned and h NaN-filled before the call (step 0 has no history) == the clean run."""
    B = 6
    x0 = images(B, 3, 8, 10)
    rows = _rows("sde-dpmsolver++", n=10)
    st = side_stream()
    outs = []
    for poison in (False, True):
        es, ef, _ = _tiny_pair(max_batch=B, seeds=(71, 72))
        h0 = None
        if poison:
            for e in (es, ef):
                es.ctx.check(es.ctx.lib.dd_dev_poison_workspaces(es.ctx.handle, e.handle, st.cuda_stream))
            h0 = torch.full_like(x0, float("nan"))
        outs.append(_loop(es, ef, x0, rows, st, switch_after=3, h0=h0, flags=L.DD_DEV_FORCE_CHAINS))
        del es, ef
    assert outs[0][2] == outs[1][2] == 2
    assert torch.isfinite(outs[0][0]).all() and torch.isfinite(outs[1][1]).all()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "poisoned run differs"


@gpu
def test_invalid_multistep_calls_are_rejected_before_anything_is_enqueued():
    from duodiff_amd.engine import Model
    B = 4
    es, ef, _ = _tiny_pair(max_batch=B)
    ctx, lib = es.ctx, es.ctx.lib
    ee = Model(ctx, ModelParams.from_dict(dict(TINY, depth=3)), B)
    ee.enable_early_exit("mlp_probe_per_layer")
    x0 = images(B, 3, 8, 11)
    rows = _rows("dpmsolver++", n=3)
    st = side_stream()
    n0 = lib.dd_dev_graph_captures(ctx.handle)
    f = lambda k: np.ascontiguousarray(rows[k], np.float32)
    i = lambda k: np.ascontiguousarray(rows[k], np.int32)
    keep = {k: f(k) for k in "tabcdpq"}
    keep.update(noise=i("noise"), hist=i("hist"))
    for what, msg in (("n_steps", "n_steps"), ("h_dev", "h_dev"), ("noise_mode", "host noise"), ("early_exit", "early-exit")):
        x, h = x0.clone(), torch.zeros_like(x0)
        a = L.dd_multistep_sample_args()
        a.first, a.late, a.n_steps, a.switch_after = (ee if what == "early_exit" else es).handle, None, 0 if what == "n_steps" else 3, 3
        for k in "tabcdpq":
            setattr(a, k, keep[k].ctypes.data_as(C.POINTER(C.c_float)))
        a.noise, a.hist = (keep[k].ctypes.data_as(C.POINTER(C.c_int32)) for k in ("noise", "hist"))
        a.noise_mode = L.DD_NOISE_BUFFER if what == "noise_mode" else L.DD_NOISE_PHILOX
        a.use_graph, a.seed, a.y_dev, a.x_dev, a.B = 1, 1, None, x.data_ptr(), B
        a.h_dev = None if what == "h_dev" else h.data_ptr()
        with torch.cuda.stream(st):
            rc = lib.dd_sample_multistep(ctx.handle, C.byref(a), C.c_void_p(st.cuda_stream))
        st.synchronize()
        err = lib.dd_last_error(ctx.handle).decode()
        assert rc == L.DD_ERR_INVALID and (msg in err or (what == "noise_mode" and "noise" in err)), (what, rc, err)
        assert torch.equal(x, x0) and not h.any(), f"{what}: something was enqueued"
    assert lib.dd_dev_graph_captures(ctx.handle) == n0


@gpu
def test_fp32_engine_matches_the_oracle_driven_by_the_float64_solver():
    """20 DPM-Solver++(2M) ODE steps: the fp32 engine (device loop, fp32 rows) against the numpy oracle driven by the float64 rows of
    the same grid (max abs <= 1e-3)."""
    import oracle
    from duodiff_amd import sampler
    from duodiff_amd.engine import sample_multistep_loop
    B = 3
    cfg = dict(TINY)
    mp = ModelParams.from_dict(cfg)
    sd = synthetic_state_dict(mp, 61)
    orc = oracle.UViTOracle(mp.as_dict(), {k: v.numpy() for k, v in sd.items()})
    x0 = torch.randn(B, 3, 8, 8, generator=torch.Generator().manual_seed(12))
    ts = sampler.multistep_grid(20)
    r64 = sampler.multistep_rows("dpmsolver++", _abar()[ts], 2)
    x, h = x0.numpy().astype(np.float64), None
    for k in range(20):
        m = orc(x.astype(np.float32), np.full((B,), float(ts[k]), np.float32)).astype(np.float64)
        v = r64["a"][k] * x + r64["b"][k] * m + (r64["d"][k] * h if r64["hist"][k] else 0.0)
        h, x = r64["p"][k] * x + r64["q"][k] * m, v
    m32, _ = uvit(cfg, 61, "fp32", B)
    em = m32.engine_model(B)
    xd, hd = x0.cuda(), torch.zeros(B, 3, 8, 8, device="cuda")
    sample_multistep_loop(em.ctx, em, None, xd, hd, sampler.multistep_coefficients("dpmsolver++", ts, 2), noise="none")
    torch.cuda.synchronize()
    err = float(np.abs(xd.cpu().numpy() - x).max())
    print(f"fp32 engine vs float64 solver on the oracle, 20 steps: max abs {err:.3e} (|x| max {np.abs(x).max():.3f})")
    assert np.isfinite(err) and err <= 1e-3


@gpu
@pytest.mark.parametrize("noise", ["device", "torch_cpu"])
def test_cli_dpm_solver_end_to_end(tmp_path, noise):
    import yaml
    cfg = dict(TINY, depth=3, img_size=16)
    (tmp_path / "m.yaml").write_text(yaml.safe_dump({"model_params": cfg}))
    torch.save(dict(synthetic_state_dict(ModelParams.from_dict(cfg), 91)), tmp_path / "m.pth")
    out = tmp_path / "out"
    cmd = [sys.executable, "-m", "duodiff_amd.sampler", "--seed", "5", "--checkpoint_path", str(tmp_path / "m.pth"),
           "--config_path", str(tmp_path / "m.yaml"), "--batch_size", "3", "--parametrization", "predict_noise",
           "--output_folder", str(out), "--no_png", "--dpm_solver", "ode", "--dpm_solver_steps", "10", "--noise", noise,
           "--timesteps_save", "500"]
    r = subprocess.run(cmd, cwd=str(REPO), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    s = np.load(out / "samples.npy")
    assert s.shape == (3, 16, 16, 3) and np.isfinite(s).all()
