"""Known regions: inpainting and image-to-image starts in the device-resident loops (dd_known_region, dd_known_blend,
dd_sample_region / dd_sample_affine_region / dd_sample_multistep_region, get_samples' init_image / strength / known_image / known_mask).

CPU tests: the host rows (sampler.known_rows), the plans that start below t = 999, the command line's validation and the binding.
GPU tests (marked): the rule against a numpy fp32 restatement, the fused loops against the plain loops (mask 0), against x0 (mask 1)
and against forward + step + known_blend, chains, cuts, both kinds of guidance, the independence of z2 from z, staged inputs, stale
bytes, the rejected calls, the fp32 engine against the numpy oracle and the command line.  Bit for bit unless a bound is named.
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
from loop_support import KINDS, NULL, labels, philox_z, philox_z2, region_inputs, run_loop, run_steps, side_stream, tiny_model, uvit

gpu = pytest.mark.gpu
CELEBA_3 = REPO / "configs" / "uvit_celeba_3.yaml"


def _plan(kind, n=6, cut=0):
    """a plan of n steps that ends on the final image (cut: without its last `cut` steps): DDPM from t = n - 1 (a strength start),
    DDIM with eta 0.01 (its last pair has no real coefficient at a larger one) and the SDE solver from 999"""
    from duodiff_amd import sampler
    if kind == "ddpm":
        p = sampler.step_plan("predict_noise", strength=(n - 1) / 999)
    elif kind == "affine":
        p = sampler.step_plan(None, use_ddim=True, ddim_steps=n + 1, ddim_eta=0.01)
    else:
        p = sampler.step_plan("predict_noise", solver="sde-dpmsolver++", solver_steps=n)
    assert len(p.rows["t"]) == n
    if cut:
        p = p._replace(rows={k: v[:-cut] for k, v in p.rows.items()}, save_after=p.save_after[:-cut], lands=p.lands[:-cut])
    return p


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_known_rows_follow_the_tables():
    from duodiff_amd import sampler
    from duodiff_amd.engine import schedule_tables
    ab = schedule_tables()["alphas_bar"].astype(np.float64)
    plans = {"ddpm": (sampler.step_plan("predict_noise"), [t - 1 for t in range(999, 0, -1)]),
             "ddim6": (sampler.step_plan(None, use_ddim=True, ddim_steps=7), [832, 666, 499, 333, 166]),
             "multistep5": (sampler.step_plan("predict_noise", solver="dpmsolver++", solver_steps=5), [799, 599, 400, 200])}
    for name, (p, lands) in plans.items():
        ka, kb = sampler.known_rows(p)
        assert ka.dtype == kb.dtype == np.float32 and len(ka) == len(kb) == len(p.rows["t"]) == len(lands) + 1, name
        assert list(p.lands) == lands + [-1], name
        assert np.array_equal(ka[:-1], np.sqrt(ab[lands]).astype(np.float32)), name
        assert np.array_equal(kb[:-1], np.sqrt(1.0 - ab[lands]).astype(np.float32)), name
        assert (ka[-1], kb[-1]) == (1.0, 0.0), name
    # a DDPM run cut short of t = 0 has no final row
    ka, kb = sampler.known_rows(sampler.step_plan("predict_noise", num_steps=3))
    assert np.array_equal(ka, np.sqrt(ab[[998, 997, 996]]).astype(np.float32)) and (kb > 0).all()


@pytest.mark.parametrize("strength", [0.5, 0.25, 0.05, 1.0, None])
def test_step_plan_strength(strength):
    from duodiff_amd import sampler
    t0 = 999 if strength is None else int(round(999 * strength))
    cases = {"ddpm": dict(parametrization="predict_noise"), "original": dict(parametrization="predict_original"),
             "ddim": dict(parametrization=None, use_ddim=True, ddim_steps=20),
             "ode": dict(parametrization="predict_noise", solver="dpmsolver++", solver_steps=20),
             "sde": dict(parametrization="predict_original", solver="sde-dpmsolver++", solver_steps=7)}
    for name, kw in cases.items():
        p = sampler.step_plan(**kw, strength=strength)
        base = sampler.step_plan(**kw)
        t = p.rows["t"]
        assert t[0] == t0, name
        assert (np.diff(t) < 0).all() and (t >= 0).all(), name
        assert p.lands[-1] == -1 and p.rows["noise"][-1] == 0, name                     # ends on the final image, as before
        if name in ("ddpm", "original"):
            assert t[-1] == 0 and len(t) == t0 + 1
        else:
            assert len(t) == len(base.rows["t"]), name                                  # the same number of steps
        if name == "ddim":
            ts = np.linspace(0, t0, 20).astype(int)[::-1]
            assert t.tolist() == ts[:-1].tolist()
            want = [sampler.affine_coefficients("ddim", int(a), int(b), 0.0) for a, b in zip(ts[:-1], ts[1:])]
            assert p.rows["a"].tobytes() == np.array([w[0] for w in want], np.float32).tobytes()
        if name == "ode":
            assert t.tolist() == np.linspace(t0, 0, 21).round().astype(int)[:-1].tolist()
        if t0 == 999:
            assert p.kind == base.kind and p.save_after == base.save_after and p.switch_after == base.switch_after
            assert sorted(p.rows) == sorted(base.rows) and all(p.rows[k].tobytes() == base.rows[k].tobytes() for k in p.rows), name


def test_step_plan_strength_switch_and_errors():
    from duodiff_amd import sampler
    # the late model takes over after the step at t == 1000 - t_switch, wherever the loop starts
    p = sampler.step_plan("predict_noise", has_late=True, t_switch=700, strength=0.5)
    assert p.rows["t"][0] == 500 and p.rows["t"][p.switch_after - 1] == 300
    assert sampler.step_plan("predict_noise", has_late=True, t_switch=300, strength=0.5).switch_after == 0     # t = 700 is behind the start
    p = sampler.step_plan("predict_noise", has_late=True, t_switch=700, strength=0.5, solver="dpmsolver++", solver_steps=10)
    assert p.switch_after == min(k for k, t in enumerate(p.rows["t"]) if t < 300)
    for bad in (0, 0.0, -0.1, 1.01, float("nan"), "0.5"):
        with pytest.raises(ValueError, match="strength"):
            sampler.step_plan("predict_noise", strength=bad)
    with pytest.raises(ValueError, match="do not fit"):
        sampler.step_plan(None, use_ddim=True, ddim_steps=50, strength=0.02)
    with pytest.raises(ValueError, match="do not fit"):
        sampler.step_plan("predict_noise", solver="dpmsolver++", solver_steps=30, strength=0.02)


def _cli_files(tmp_path, in_chans=3):
    import yaml
    cfg = dict(TINY, in_chans=in_chans)
    (tmp_path / "m.yaml").write_text(yaml.safe_dump({"model_params": cfg}))
    rng = np.random.default_rng(0)
    np.save(tmp_path / "img.npy", rng.standard_normal((1, in_chans, 8, 8)).astype(np.float32))
    np.save(tmp_path / "img_b.npy", rng.standard_normal((2, in_chans, 8, 8)).astype(np.float32))
    np.save(tmp_path / "img16.npy", rng.standard_normal((1, in_chans, 16, 16)).astype(np.float32))
    np.save(tmp_path / "mask.npy", (rng.random((1, 1, 8, 8)) < 0.5).astype(np.float32))
    np.save(tmp_path / "mask3.npy", np.ones((1, 3, 8, 8), np.float32))
    np.save(tmp_path / "mask_big.npy", np.full((1, 1, 8, 8), 1.5, np.float32))
    from matplotlib import pyplot as plt
    plt.imsave(tmp_path / "img.png", rng.random((8, 8, 3)))
    return ["--checkpoint_path", "/nonexistent.pth", "--batch_size", "2", "--parametrization", "predict_noise",
            "--output_folder", str(tmp_path / "out"), "--config_path", str(tmp_path / "m.yaml")]


@pytest.mark.parametrize("extra,match", [
    (["--known_mask", "mask.npy"], "go together"),                                       # a mask without an image
    (["--known_image", "img.npy"], "go together"),
    (["--init_image", "img.npy"], "go together"),
    (["--strength", "0.5"], "go together"),
    (["--init_image", "img.npy", "--strength", "0"], "outside"),
    (["--init_image", "img.npy", "--strength", "1.5"], "outside"),
    (["--init_image", "img.npy", "--strength", "-0.2"], "outside"),
    (["--init_image", "img16.npy", "--strength", "0.5"], "does not match"),              # shape mismatches
    (["--known_image", "img.npy", "--known_mask", "mask3.npy"], "does not match"),
    (["--known_image", "img16.npy", "--known_mask", "mask.npy"], "does not match"),
    (["--known_image", "img.npy", "--known_mask", "mask_big.npy"], r"outside \[0, 1\]"),
    (["--known_image", "img.txt", "--known_mask", "mask.npy"], "npy or .png"),
])
def test_cli_rejects_invalid_region_options_before_any_gpu_work(tmp_path, extra, match):
    from duodiff_amd import sampler
    argv = _cli_files(tmp_path)
    extra = [str(tmp_path / v) if v.endswith((".npy", ".png", ".txt")) else v for v in extra]
    with pytest.raises(ValueError, match=match):
        sampler.main(argv + extra)          # (the checkpoint does not exist: passing validation would fail differently)


def test_cli_rejects_png_for_four_channels_and_for_latents(tmp_path):
    from duodiff_amd import dist, sampler
    argv = _cli_files(tmp_path, in_chans=4)
    with pytest.raises(ValueError, match="in_chans = 3"):
        sampler.main(argv + ["--init_image", str(tmp_path / "img.png"), "--strength", "0.5"])
    argv[argv.index("--config_path") + 1] = str(REPO / "configs" / "uvit_imagenet256.yaml")       # a latent model
    with pytest.raises(ValueError, match="latents only"):
        sampler.main(argv + ["--known_image", str(tmp_path / "img.png"), "--known_mask", str(tmp_path / "mask.npy")])
    with pytest.raises(ValueError, match="single-GPU"):
        dist.main(_cli_files(tmp_path) + ["--init_image", str(tmp_path / "img.npy"), "--strength", "0.5"])


def test_cli_loads_valid_region_files(tmp_path):
    from duodiff_amd import sampler
    argv = _cli_files(tmp_path)
    a = sampler.get_args(argv)
    assert (a.init_image, a.strength, a.known_image, a.known_mask) == (None, None, None, None)
    assert sampler.validate_region(a, load_config(tmp_path / "m.yaml")) == dict(init_image=None, strength=None, known_image=None,
                                                                                known_mask=None)
    a = sampler.get_args(argv + ["--init_image", str(tmp_path / "img.png"), "--strength", "0.3", "--known_image",
                                 str(tmp_path / "img_b.npy"), "--known_mask", str(tmp_path / "img.png")])
    kw = sampler.validate_region(a, load_config(tmp_path / "m.yaml"))
    assert kw["strength"] == 0.3 and kw["init_image"].shape == (1, 3, 8, 8) and kw["known_image"].shape == (2, 3, 8, 8)
    assert kw["known_mask"].shape == (1, 1, 8, 8)
    assert -1 <= kw["init_image"].min() < 0 < kw["init_image"].max() <= 1               # 2 v - 1
    assert 0 <= kw["known_mask"].min() and kw["known_mask"].max() <= 1                  # the first channel, unmapped
    assert np.abs(kw["known_mask"][0, 0] - (kw["init_image"][0, 0] + 1) / 2).max() <= 1e-6   # (2 v - 1 rounds: not bit for bit)


def test_lib_binds_the_region_entry_points():
    assert L.ABI_VERSION == 6
    assert C.sizeof(L.dd_known_region) == 32 and L.dd_known_region.kb.offset == 24
    for name, args in (("dd_sample_region", L.dd_sample_args), ("dd_sample_affine_region", L.dd_affine_sample_args),
                       ("dd_sample_multistep_region", L.dd_multistep_sample_args)):
        assert L.SIGNATURES[name][1] == [C.c_void_p, C.POINTER(args), C.POINTER(L.dd_guidance), C.POINTER(L.dd_autoguidance),
                                         C.POINTER(L.dd_known_region), C.c_void_p]
    assert len(L.SIGNATURES["dd_known_blend"][1]) == 12
    lib = L.load()
    assert lib.dd_abi_version() == 6
    for name in ("dd_known_blend", "dd_sample_region", "dd_sample_affine_region", "dd_sample_multistep_region"):
        assert hasattr(lib, name)


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def _counter(kind, plan, k):
    """the Philox counter of step k: the timestep in the DDPM loop, the step index in a table-driven one"""
    return int(plan.rows["t"][k]) if kind == "ddpm" else k


def _blend_numpy(x, x0, m, z2, ka, kb):
    """the rule, op by op in float32"""
    x, x0, m = (np.asarray(v, np.float32) for v in (x, x0, m))
    ka, kb = np.float32(ka), np.float32(kb)
    with np.errstate(invalid="ignore"):
        kn = ka * x0
        if kb != 0 and z2 is not None:
            kn = kn + kb * np.asarray(z2, np.float32)
        out = m * kn + (np.float32(1) - m) * x
    assert out.dtype == np.float32
    return np.where(m == 0, x, out)


@gpu
@pytest.mark.parametrize("shape", [(2, 3, 8, 8), (3, 4, 5, 5), (1, 1, 19, 19)])
def test_known_blend_kernel_bit_exact(shape):
    """dd_known_blend == the numpy restatement for masks {0, 1, 0.25}, kb = 0 and != 0, with and without z2, element counts that are
    no multiple of the block (300, 361) and one that is; a NaN in x0 under m == 0 does not reach x'."""
    from duodiff_amd.engine import Context
    ctx = Context.get()
    B, Cc, S, _ = shape
    g = torch.Generator().manual_seed(21)
    x, x0, z2 = (torch.randn(shape, generator=g) for _ in range(3))
    mask = torch.tensor([0.0, 1.0, 0.25])[torch.randint(0, 3, (B, 1, S, S), generator=g)]
    mask[0, 0, 0, :3] = torch.tensor([0.0, 1.0, 0.25])
    x0 = torch.where((mask == 0).expand(shape) & (torch.rand(shape, generator=g) < 0.5), torch.tensor(float("nan")), x0)
    assert torch.isnan(x0).any()
    for ka, kb in ((0.83, 0.0), (0.61, 0.79), (1.0, 0.0), (0.0, 1.0)):
        for with_z in (True, False):
            out = ctx.known_blend(x.cuda(), x0.cuda(), mask.cuda(), z2.cuda() if with_z else None, ka, kb)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            want = _blend_numpy(x.numpy(), x0.numpy(), mask.numpy(), z2.numpy() if with_z else None, ka, kb)
            keep = np.broadcast_to(mask.numpy() == 0, shape)
            assert np.array_equal(got[keep].view(np.uint32), x.numpy()[keep].view(np.uint32)), "m == 0 must keep x' bit for bit"
            assert np.isfinite(got).all()
            assert np.array_equal(got, want), (ka, kb, with_z)
            ones = np.broadcast_to(mask.numpy() == 1, shape)
            kn = np.float32(ka) * x0.numpy()[ones]
            if kb != 0 and with_z:
                kn = kn + np.float32(kb) * z2.numpy()[ones]
            assert np.array_equal(got[ones], kn), "m == 1 must give kn"
    xi = x.cuda()                                                  # in place
    ctx.known_blend(xi, x0.cuda(), mask.cuda(), z2.cuda(), 0.61, 0.79, out=xi)
    torch.cuda.synchronize()
    assert np.array_equal(xi.cpu().numpy(), _blend_numpy(x.numpy(), x0.numpy(), mask.numpy(), z2.numpy(), 0.61, 0.79))
    with pytest.raises(ValueError):
        ctx.check(ctx.lib.dd_known_blend(ctx.handle, None, None, None, None, 1.0, 0.0, None, 1, 1, 1, None))


@gpu
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_zero_mask_equals_the_plain_loop(kind, guided):
    """m == 0 everywhere (x0 NaN-filled): the region loop == the plain loop of the same arguments, bit for bit, x and h; also with
    classifier-free guidance on a class-conditional model."""
    B = 2
    m = tiny_model(2 * B, num_classes=11) if guided else tiny_model(B)
    x, x0, mask = region_inputs(B, 31, mask=0.0)
    x0.fill_(float("nan"))
    y = torch.tensor([3, 7]).cuda() if guided else None
    guidance = (0.6, NULL) if guided else None
    plan, st = _plan(kind), side_stream()
    xp, hp, _ = run_loop(kind, m, x, plan, st, y=y, guidance=guidance)
    xr, hr, _ = run_loop(kind, m, x, plan, st, y=y, guidance=guidance, region=(x0, mask))
    assert torch.isfinite(xp).all() and not torch.equal(xp, x)
    assert torch.equal(xr, xp) and torch.equal(hr, hp), "an all-zero mask changed the loop"


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_one_mask_gives_the_known_image(kind):
    """m == 1 everywhere: the result is x0 itself; a run cut one step early ends on ka x0 + kb z2 of its last step."""
    from duodiff_amd import sampler
    B = 2
    m = tiny_model(B)
    x, x0, mask = region_inputs(B, 32, mask=1.0)
    st = side_stream()
    plan = _plan(kind)
    xr, _, _ = run_loop(kind, m, x, plan, st, region=(x0, mask))
    assert torch.equal(xr, x0), "the known pixels of the result are not x0"
    short = _plan(kind, cut=1)
    xs, _, _ = run_loop(kind, m, x, short, st, region=(x0, mask))
    ka, kb = sampler.known_rows(short)
    k = len(ka) - 1
    assert kb[k] > 0 and ka[k] < 1
    z2 = philox_z2(m, x, _counter(kind, short, k), 5, st)
    want = ka[k] * x0.cpu().numpy() + kb[k] * z2.cpu().numpy()
    assert want.dtype == np.float32 and np.array_equal(xs.cpu().numpy(), want)


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_loop_forms_agree(kind):
    """A checkerboard mask with some 0.5 entries: graph replay == eager launches == forward + the unfused step + known_blend."""
    B = 2
    m = tiny_model(B)
    x, x0, mask = region_inputs(B, 33)
    assert set(mask.unique().tolist()) == {0.0, 0.5, 1.0}
    plan, st = _plan(kind), side_stream()
    xg, hg, _ = run_loop(kind, m, x, plan, st, region=(x0, mask), use_graph=True)
    xe, he, _ = run_loop(kind, m, x, plan, st, region=(x0, mask), use_graph=False)
    xs, hs = run_steps(kind, m, x, plan, st, region=(x0, mask))
    xp, _, _ = run_loop(kind, m, x, plan, st)
    assert torch.isfinite(xg).all() and not torch.equal(xg, xp), "the region changed nothing"
    assert torch.equal(xg, xe) and torch.equal(hg, he), "graph replay differs from eager launches"
    assert torch.equal(xg, xs), "device loop differs from forward + step + known_blend"
    if kind == "multistep":
        assert torch.equal(hg, hs), "the history register differs"
    keep = (mask == 1).expand_as(x0)
    assert torch.equal(xg[keep], x0[keep])
    # DD_NOISE_NONE: neither c z nor kb z2 is added
    xn, _, _ = run_loop(kind, m, x, plan, st, region=(x0, mask), noise="none")
    plan_nz = plan._replace(rows=dict(plan.rows, noise=np.zeros_like(plan.rows["noise"])))
    xns, _ = run_steps(kind, m, x, plan_nz, st, region=(x0, mask), with_z2=False)
    assert torch.equal(xn, xns), "DD_NOISE_NONE differs from the steps without z and z2"


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_two_chains_and_cut_loops(kind):
    """B = 6 with the chain split forced: two chains == one chain, and a loop cut into calls (counter_base and h carried) == the uncut one."""
    B = 6
    m = tiny_model(B)
    x, x0, mask = region_inputs(B, 34)
    plan, st = _plan(kind, n=7), side_stream()
    x2, h2, c2 = run_loop(kind, m, x, plan, st, region=(x0, mask), flags=L.DD_DEV_FORCE_CHAINS)
    x1, h1, c1 = run_loop(kind, m, x, plan, st, region=(x0, mask), flags=L.DD_DEV_NO_CHAINS)
    assert (c2, c1) == (2, 1)
    assert torch.isfinite(x1).all() and torch.equal(x2, x1) and torch.equal(h2, h1), "two chains differ from one"
    xc, hc, _ = run_loop(kind, m, x, plan, st, region=(x0, mask), flags=L.DD_DEV_FORCE_CHAINS, cuts=(2, 3, 6))
    assert torch.equal(xc, x2) and torch.equal(hc, h2), "a cut loop differs from the uncut loop"


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_guided_region_equals_the_steps(kind):
    """Classifier-free guidance with a region, chains forced: == forward_guided + step + blend (both rows of an image carry x'')."""
    B = 6
    m = tiny_model(2 * B, num_classes=11)
    x, x0, mask = region_inputs(B, 35)
    y = labels(B, NULL, 6)
    plan, st = _plan(kind, n=5), side_stream()
    xg, hg, c = run_loop(kind, m, x, plan, st, region=(x0, mask), y=y, guidance=(0.4, NULL), flags=L.DD_DEV_FORCE_CHAINS)
    xs, hs = run_steps(kind, m, x, plan, st, region=(x0, mask), y=y, guidance=(0.4, NULL))
    assert c == 2 and torch.isfinite(xg).all()
    assert torch.equal(xg, xs) and torch.equal(hg, hs), "guided region loop differs from forward_guided + step + blend"


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_autoguided_region_equals_the_steps(kind):
    """Autoguidance of the depth-3 model by the depth-1 one, with a region, chains forced: == forward_autoguided + step + blend."""
    from duodiff_amd.engine import Autoguidance
    B = 6
    guide, m = tiny_model(B, seed=41, depth=1), tiny_model(B, seed=42)
    x, x0, mask = region_inputs(B, 36)
    plan, st = _plan(kind, n=5), side_stream()
    ag = Autoguidance(guide, 0.7)
    xg, hg, c = run_loop(kind, m, x, plan, st, region=(x0, mask), guidance=ag, flags=L.DD_DEV_FORCE_CHAINS)
    xs, hs = run_steps(kind, m, x, plan, st, region=(x0, mask), guidance=ag)
    xu, _, _ = run_loop(kind, m, x, plan, st, region=(x0, mask))
    assert c == 2 and torch.isfinite(xg).all() and not torch.equal(xg, xu)
    assert torch.equal(xg, xs) and torch.equal(hg, hs), "autoguided region loop differs from forward_autoguided + step + blend"


@gpu
def test_z2_is_independent_of_z():
    """z2 differs from z at the same step, and over the B C S S values of 8 steps their sample correlation is below 5 / sqrt(N):
    independent normals give a standard deviation of 1 / sqrt(N)."""
    B = 2
    m = tiny_model(B)
    x, _, _ = region_inputs(B, 37)
    st = side_stream()
    zs, z2s = [], []
    for k in range(8):
        z, z2 = philox_z(m, x, k, 9, st), philox_z2(m, x, k, 9, st)
        assert not torch.equal(z, z2)
        zs.append(z.cpu().numpy().ravel())
        z2s.append(z2.cpu().numpy().ravel())
    a, b = np.concatenate(zs).astype(np.float64), np.concatenate(z2s).astype(np.float64)
    n = a.size
    assert n == 8 * B * 3 * 8 * 8
    r = float(np.corrcoef(a, b)[0, 1])
    print(f"corr(z, z2) over {n} values: {r:.4f} (bound {5 / np.sqrt(n):.4f}); z2 mean {b.mean():.3f} std {b.std():.3f}")
    assert abs(r) < 5 / np.sqrt(n)
    assert abs(b.mean()) < 5 / np.sqrt(n) and abs(b.std() - 1) < 5 / np.sqrt(2 * n)     # N(0, 1): the mean's and the deviation's own spread
    assert np.array_equal(philox_z2(m, x, 3, 9, st).cpu().numpy().ravel(), z2s[3])     # a pure function of (seed, pixel, counter)


@gpu
def test_second_call_with_other_tensors():
    """A second call with another x0 / mask of the same shape gives that call's own step-by-step result, replaying the graphs of the first."""
    B = 2
    m = tiny_model(B)
    plan, st = _plan("affine"), side_stream()
    x, x0a, ma = region_inputs(B, 38)
    _, x0b, _ = region_inputs(B, 39)
    mb = (1 - ma).contiguous()
    lib, h = m.ctx.lib, m.ctx.handle
    ra, _, _ = run_loop("affine", m, x, plan, st, region=(x0a, ma))
    n0 = lib.dd_dev_graph_captures(h)
    rb, _, _ = run_loop("affine", m, x, plan, st, region=(x0b, mb))
    assert lib.dd_dev_graph_captures(h) == n0, "the second call re-captured a graph"
    re_, _, _ = run_loop("affine", m, x, plan, st, region=(x0b, mb), use_graph=False)
    sa, _ = run_steps("affine", m, x, plan, st, region=(x0a, ma))
    sb, _ = run_steps("affine", m, x, plan, st, region=(x0b, mb))
    assert not torch.equal(ra, rb)
    assert torch.equal(ra, sa) and torch.equal(rb, sb) and torch.equal(re_, sb)
    # a plain call in between keeps its own graph and result
    p1, _, _ = run_loop("affine", m, x, plan, st)
    ra2, _, _ = run_loop("affine", m, x, plan, st, region=(x0a, ma))
    p2, _, _ = run_loop("affine", m, x, plan, st)
    assert torch.equal(p1, p2) and torch.equal(ra2, ra) and not torch.equal(p1, ra)


@gpu
def test_poisoned_workspaces_and_history_with_a_region():
    """Both chains' workspaces NaN-poisoned before the call, on fresh models: == the clean run (multistep, chains forced)."""
    B = 6
    x, x0, mask = region_inputs(B, 40)
    plan, st = _plan("multistep", n=8), side_stream()
    outs = []
    for poison in (False, True):
        m = tiny_model(B, seed=71)
        if poison:
            m.ctx.check(m.ctx.lib.dd_dev_poison_workspaces(m.ctx.handle, m.handle, st.cuda_stream))
        outs.append(run_loop("multistep", m, x, plan, st, region=(x0, mask), flags=L.DD_DEV_FORCE_CHAINS))
        del m
    assert outs[0][2] == outs[1][2] == 2
    assert torch.isfinite(outs[0][0]).all() and torch.isfinite(outs[1][1]).all()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "poisoned run differs"


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_invalid_region_calls_are_rejected_before_anything_is_enqueued(kind):
    from duodiff_amd.engine import Model
    B = 2
    m, guide = tiny_model(B), tiny_model(B, seed=41, depth=1)
    ctx, lib = m.ctx, m.ctx.lib
    ee = Model(ctx, ModelParams.from_dict(dict(TINY)), B)
    ee.enable_early_exit("mlp_probe_per_layer")
    x_in, x0, mask = region_inputs(B, 41)
    plan, st = _plan(kind, n=3), side_stream()
    tab = {k: np.ascontiguousarray(v, np.int32 if k in ("noise", "hist") else np.float32) for k, v in plan.rows.items()}
    ka, kb = np.ones(3, np.float32), np.zeros(3, np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    n0 = lib.dd_dev_graph_captures(ctx.handle)
    cases = [("null_region", "dd_known_region"), ("x0", "member"), ("mask", "member"), ("ka", "member"), ("kb", "member"),
             ("host_noise", "noise"), ("early_exit", "early-exit"), ("both", "exclusive"),
             ("batch", "batch size"), ("labels", "labels"), ("guided_uncond", "class-conditional"), ("x_null", "null tensor")]
    for what, msg in cases:
        x, h = x_in.clone(), torch.zeros_like(x_in)
        first = ee if what == "early_exit" else m
        if kind == "ddpm":
            a = L.dd_sample_args()
            a.first, a.late, a.t_start, a.t_end = first.handle, None, 2, 0
        else:
            a = L.dd_affine_sample_args() if kind == "affine" else L.dd_multistep_sample_args()
            a.first, a.late, a.n_steps, a.switch_after = first.handle, None, 3, 3
            for k in tab:
                setattr(a, k, tab[k].ctypes.data_as(C.POINTER(C.c_int32 if k in ("noise", "hist") else C.c_float)))
            if kind == "multistep":
                a.h_dev = h.data_ptr()
        a.noise_mode = L.DD_NOISE_BUFFER if what == "host_noise" else L.DD_NOISE_PHILOX
        a.use_graph, a.seed, a.B = 1, 1, (B + 1 if what == "batch" else B)
        a.y_dev = torch.zeros(B, dtype=torch.int64, device="cuda").data_ptr() if what == "labels" else None
        a.x_dev = None if what == "x_null" else x.data_ptr()
        kr = L.dd_known_region(None if what == "x0" else x0.data_ptr(), None if what == "mask" else mask.data_ptr(),
                               None if what == "ka" else fp(ka), None if what == "kb" else fp(kb))
        g = L.dd_guidance(0.5, NULL) if what in ("both", "guided_uncond") else None
        ag = L.dd_autoguidance(guide.handle, 0.5) if what == "both" else None
        fn = getattr(lib, {"ddpm": "dd_sample_region", "affine": "dd_sample_affine_region", "multistep": "dd_sample_multistep_region"}[kind])
        with torch.cuda.stream(st):
            rc = fn(ctx.handle, C.byref(a), None if g is None else C.byref(g), None if ag is None else C.byref(ag),
                    None if what == "null_region" else C.byref(kr), C.c_void_p(st.cuda_stream))
        st.synchronize()
        err = lib.dd_last_error(ctx.handle).decode()
        assert rc == L.DD_ERR_INVALID and msg in err, (what, rc, err)
        assert torch.equal(x, x_in) and not h.any(), f"{what}: something was enqueued"
    assert lib.dd_dev_graph_captures(ctx.handle) == n0


@gpu
def test_loop_rejections_keep_their_order():
    """Calls that break two rules at once fail on the rule the loops check first (the texts in the order of the checks in loops.hip: the
    region's own rules, the multistep loop's early-exit exclusion, the models, the loop's tensors and ranges, the noise mode)."""
    from duodiff_amd.engine import Model
    B = 2
    m, guide = tiny_model(B), tiny_model(B, seed=41, depth=1)
    ctx, lib = m.ctx, m.ctx.lib
    ee = Model(ctx, ModelParams.from_dict(dict(TINY)), B)
    ee.enable_early_exit("mlp_probe_per_layer")
    x_in, x0, mask = region_inputs(B, 43)
    x, h, st = x_in.clone(), torch.zeros_like(x_in), side_stream()
    tab = {k: np.ascontiguousarray(v, np.int32 if k in ("noise", "hist") else np.float32) for k, v in _plan("multistep", n=3).rows.items()}
    ka, kb = np.ones(3, np.float32), np.zeros(3, np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    kr = L.dd_known_region(x0.data_ptr(), mask.data_ptr(), fp(ka), fp(kb))
    g, ag = L.dd_guidance(0.5, NULL), L.dd_autoguidance(guide.handle, 0.5)

    def args(kind, first=m, **fields):
        if kind == "ddpm":
            a = L.dd_sample_args()
            a.t_start, a.t_end = 2, 0
        else:
            a = L.dd_affine_sample_args() if kind == "affine" else L.dd_multistep_sample_args()
            a.n_steps, a.switch_after = 3, 3
            for k in "tabc" + ("dpq" if kind == "multistep" else ""):
                setattr(a, k, fp(tab[k]))
            for k in ("noise",) + (("hist",) if kind == "multistep" else ()):
                setattr(a, k, tab[k].ctypes.data_as(C.POINTER(C.c_int32)))
            if kind == "multistep":
                a.h_dev = h.data_ptr()
        a.first, a.late, a.y_dev, a.x_dev = first.handle, None, None, x.data_ptr()
        a.noise_mode, a.use_graph, a.seed, a.B = L.DD_NOISE_PHILOX, 1, 1, B
        for k, v in fields.items():
            setattr(a, k, v)
        return a

    both = (C.byref(g), C.byref(ag), C.byref(kr))
    cases = [(f"dd_sample{k}_region", args(kind, noise_mode=L.DD_NOISE_BUFFER), both, "classifier-free guidance and autoguidance are exclusive")
             for k, kind in (("", "ddpm"), ("_affine", "affine"), ("_multistep", "multistep"))]
    cases += [("dd_sample_multistep_region", args("multistep", ee), (None, None, None), "null dd_known_region"),
              ("dd_sample_multistep", args("multistep", ee, h_dev=None), (), "the multistep loop is not supported for early-exit models"),
              ("dd_sample_affine", args("affine", x_dev=None, n_steps=0), (), "null tensor / table"),
              ("dd_sample", args("ddpm", t_start=1, t_end=2, noise_mode=L.DD_NOISE_BUFFER), (), "need 999 >= t_start >= t_end >= 0")]
    n0 = lib.dd_dev_graph_captures(ctx.handle)
    for name, a, extra, msg in cases:
        with torch.cuda.stream(st):
            rc = getattr(lib, name)(ctx.handle, C.byref(a), *extra, C.c_void_p(st.cuda_stream))
        err = lib.dd_last_error(ctx.handle).decode()
        print(f"{name}: rc {rc}, {err!r}")
        assert rc == L.DD_ERR_INVALID and err == msg, (name, rc, err)
    st.synchronize()
    assert torch.equal(x, x_in) and not h.any() and lib.dd_dev_graph_captures(ctx.handle) == n0, "something was enqueued"


@gpu
def test_fp32_engine_matches_the_oracle_with_a_half_image_mask():
    """8 DDIM steps with the left half of the image known: the fp32 engine (device loop) against the numpy oracle driven by the
    extracted z / z2 and a numpy restatement of the rule in float64 (max abs <= 1e-3, the multistep rollout's tolerance: the blend is a
    select or a convex combination and adds no error growth)."""
    import oracle
    B = 3
    cfg = dict(TINY)
    mp = ModelParams.from_dict(cfg)
    sd = synthetic_state_dict(mp, 61)
    orc = oracle.UViTOracle(mp.as_dict(), {k: v.numpy() for k, v in sd.items()})
    em = uvit(cfg, 61, "fp32", B)[0].engine_model(B)
    from duodiff_amd import sampler
    plan = sampler.step_plan(None, use_ddim=True, ddim_steps=9, ddim_eta=0.01)
    assert len(plan.rows["t"]) == 8
    ka, kb = sampler.known_rows(plan)
    xd, x0, mask = region_inputs(B, 62, mask="half")
    st = side_stream()
    x, k0, mk = xd.cpu().numpy().astype(np.float64), x0.cpu().numpy().astype(np.float64), mask.cpu().numpy().astype(np.float64)
    r = plan.rows
    for k in range(8):
        eps = orc(x.astype(np.float32), np.full((B,), float(r["t"][k]), np.float32)).astype(np.float64)
        v = float(r["a"][k]) * x + float(r["b"][k]) * eps
        if r["noise"][k]:
            v = v + float(r["c"][k]) * philox_z(em, xd, k, 5, st).cpu().numpy().astype(np.float64)
        kn = float(ka[k]) * k0
        if kb[k] != 0:
            kn = kn + float(kb[k]) * philox_z2(em, xd, k, 5, st).cpu().numpy().astype(np.float64)
        x = np.where(mk == 0, v, mk * kn + (1 - mk) * v)
    got, _, _ = run_loop("affine", em, xd, plan, st, region=(x0, mask))
    err = float(np.abs(got.cpu().numpy() - x).max())
    print(f"fp32 engine vs the oracle, 8 DDIM steps with a half-image mask: max abs {err:.3e} (|x| max {np.abs(x).max():.3f})")
    assert np.isfinite(err) and err <= 1e-3
    assert np.array_equal(got.cpu().numpy()[..., :4], x0.cpu().numpy()[..., :4])


@gpu
def test_celeba_width_two_real_chains():
    """embed_dim 512, depth 3, 64 x 64, B = 32 (two real chains), 3 DDPM steps in bf16 == forward + ddpm_step + known_blend."""
    from duodiff_amd import sampler
    B = 32
    m = uvit(load_config(CELEBA_3), 51, "bf16", B)[0].engine_model(B)
    x, x0, mask = region_inputs(B, 42, S=64)
    plan, st = sampler.step_plan("predict_noise", num_steps=3), side_stream()
    xg, _, chains = run_loop("ddpm", m, x, plan, st, region=(x0, mask))
    xs, _ = run_steps("ddpm", m, x, plan, st, region=(x0, mask))
    xp, _, _ = run_loop("ddpm", m, x, plan, st)
    assert chains == 2 and torch.isfinite(xg).all() and not torch.equal(xg, xp)
    assert torch.equal(xg, xs), "the product path differs from forward + ddpm_step + known_blend"


def _cli(tmp_path, *extra):
    import yaml
    cfg = dict(TINY)
    (tmp_path / "m.yaml").write_text(yaml.safe_dump({"model_params": cfg}))
    torch.save(dict(synthetic_state_dict(ModelParams.from_dict(cfg), 91)), tmp_path / "m.pth")
    out = tmp_path / "out"
    cmd = [sys.executable, "-m", "duodiff_amd.sampler", "--seed", "5", "--checkpoint_path", str(tmp_path / "m.pth"),
           "--config_path", str(tmp_path / "m.yaml"), "--batch_size", "3", "--parametrization", "predict_noise",
           "--output_folder", str(out), "--no_png", *extra]
    r = subprocess.run(cmd, cwd=str(REPO), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(out / "samples.npy")


@gpu
@pytest.mark.parametrize("noise", ["device", "torch_cpu"])
def test_cli_inpainting_end_to_end(tmp_path, noise):
    """--known_image / --known_mask (.npy): the known pixels of samples.npy equal (x0 + 1) / 2."""
    rng = np.random.default_rng(1)
    x0 = rng.uniform(-1, 1, (1, 3, 8, 8)).astype(np.float32)
    mask = np.zeros((3, 1, 8, 8), np.float32)
    mask[:, :, 2:6, 1:7] = 1
    mask[1] = 1 - mask[1]
    np.save(tmp_path / "x0.npy", x0)
    np.save(tmp_path / "mask.npy", mask)
    s = _cli(tmp_path, "--use_ddim", "--ddim_steps", "8", "--noise", noise, "--known_image", str(tmp_path / "x0.npy"),
             "--known_mask", str(tmp_path / "mask.npy"))
    assert s.shape == (3, 8, 8, 3) and np.isfinite(s).all()
    want = np.broadcast_to(((x0 + np.float32(1)) / np.float32(2)).transpose(0, 2, 3, 1), s.shape)
    keep = np.broadcast_to(mask.transpose(0, 2, 3, 1) == 1, s.shape)
    assert np.array_equal(s[keep], want[keep])
    assert not np.array_equal(s[~keep], want[~keep])


@gpu
def test_cli_strength_equals_get_samples(tmp_path):
    """--init_image / --strength 0.5 with DDIM == get_samples called directly; strength 1 is the present start."""
    from duodiff_amd import sampler
    rng = np.random.default_rng(2)
    x0 = rng.uniform(-1, 1, (3, 3, 8, 8)).astype(np.float32)
    np.save(tmp_path / "x0.npy", x0)
    s = _cli(tmp_path, "--use_ddim", "--ddim_steps", "8", "--init_image", str(tmp_path / "x0.npy"), "--strength", "0.5")
    model = uvit(dict(TINY), 91, "bf16", 3)[0]
    kw = dict(model=model, batch_size=3, postprocessing=sampler.predict_noise_postprocessing, seed=5, num_channels=3, sample_height=8,
              sample_width=8, use_ddim=True, ddim_steps=8, noise="device")
    direct, _ = sampler.get_samples(**kw, init_image=x0, strength=0.5)
    assert s.shape == (3, 8, 8, 3) and np.array_equal(s, direct)
    plain, _ = sampler.get_samples(**kw)
    full, _ = sampler.get_samples(**kw, init_image=x0, strength=1.0)
    assert np.array_equal(full, plain) and not np.array_equal(direct, plain)
