"""Autoguidance: eps = eps_main + s (eps_main - eps_guide), the main model guided by a weaker model of the same image geometry, fused
into the step kernels (dd_forward_autoguided, dd_sample_autoguided, dd_sample_affine_autoguided, dd_sample_multistep_autoguided) and
the sampler options --autoguidance_scale / --guide_config_path / --guide_checkpoint_path.

CPU tests: the command line and the ctypes binding.  GPU tests (marked): the autoguided eps against the numpy oracle's two forwards
combined in fp32, scale 0 and "the guide runs the step" against the unguided loops bit for bit, the DuoDiff call, the loops against
their own building blocks, chains, graph keys, stale workspace bytes, argument errors, the CLI against an oracle rollout.
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
from duodiff_amd.engine import Autoguidance
from duodiff_amd.weights import synthetic_state_dict
from loop_support import KINDS, celeba_pair, cli_argv, engine_pair, eps_rms_bound, first_rows, imagenet256_pair, images, labels
from loop_support import run_first_steps, run_steps, side_stream, uvit

gpu = pytest.mark.gpu

CONFIGS = REPO / "configs"
F32 = np.float32


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_cli_autoguidance_options_and_defaults():
    from duodiff_amd import sampler
    a = sampler.get_args(cli_argv(CONFIGS / "uvit_celeba_3.yaml"))
    assert a.autoguidance_scale is None and a.guide_config_path is None and a.guide_checkpoint_path is None
    a = sampler.get_args(cli_argv(CONFIGS / "uvit_celeba_3.yaml", "--autoguidance_scale", "1.5", "--guide_config_path", "g.yaml",
                               "--guide_checkpoint_path", "g.pth"))
    assert a.autoguidance_scale == pytest.approx(1.5) and a.guide_config_path == "g.yaml" and a.guide_checkpoint_path == "g.pth"
    a = sampler.get_args(cli_argv(CONFIGS / "uvit_celeba_3.yaml", "--autoguidance_scale", "0"))
    assert a.autoguidance_scale == 0.0 and a.autoguidance_scale is not None       # 0 selects the autoguided path too
    assert a.cfg_scale is None


_LATE = ["--checkpoint_path_late", "/nonexistent.pth", "--config_path_late"]


@pytest.mark.parametrize("config,extra,match", [
    ("uvit_celeba_3.yaml", ["--autoguidance_scale", "nan", *_LATE, str(CONFIGS / "uvit_celeba.yaml")], "finite"),
    ("uvit_celeba_3.yaml", ["--autoguidance_scale", "inf", *_LATE, str(CONFIGS / "uvit_celeba.yaml")], "finite"),
    ("uvit_imagenet256_3.yaml", ["--autoguidance_scale", "1", "--cfg_scale", "0.4", "--class_label", "3", *_LATE,
                                 str(CONFIGS / "uvit_imagenet256.yaml")], "exclusive"),
    ("uvit_celeba_3.yaml", ["--autoguidance_scale", "1", *_LATE, str(CONFIGS / "uvit_cifar10.yaml")], "geometry"),       # 64x64 p4 against 32x32 p2
    ("uvit_celeba.yaml", ["--autoguidance_scale", "1", "--guide_config_path", str(CONFIGS / "uvit_imagenet256_3.yaml"),
                          "--guide_checkpoint_path", "/nonexistent.pth"], "geometry"),                                      # explicit guide, 4 channels
    ("uvit_celeba.yaml", ["--autoguidance_scale", "1"], "guide"),                                                          # no late model, no guide
    ("uvit_celeba.yaml", ["--autoguidance_scale", "1", "--guide_config_path", str(CONFIGS / "uvit_celeba_3.yaml")], "both"),
    ("uvit_celeba.yaml", ["--guide_config_path", str(CONFIGS / "uvit_celeba_3.yaml"), "--guide_checkpoint_path", "/nonexistent.pth"],
     "autoguidance_scale"),
])
def test_cli_rejects_invalid_autoguidance_before_any_gpu_work(tmp_path, config, extra, match):
    """main() validates the options against the YAMLs before it builds a model: no GPU is touched and no checkpoint is opened."""
    from duodiff_amd import sampler
    argv = cli_argv(CONFIGS / config, *extra)
    argv[argv.index("--output_folder") + 1] = str(tmp_path / "out")
    with pytest.raises(ValueError, match=match):
        sampler.main(argv)


def test_get_samples_rejects_invalid_autoguidance_before_any_gpu_work():
    from duodiff_amd import sampler
    from duodiff_amd.uvit import UViT
    m = UViT(**ModelParams.from_dict(dict(TINY)).as_dict())
    post = sampler.predict_noise_postprocessing
    with pytest.raises(ValueError, match="guide"):
        sampler.get_samples(m, 2, post, 0, 3, 8, 8, autoguidance_scale=1.0)                       # no late model and no explicit guide
    with pytest.raises(ValueError, match="finite"):
        sampler.get_samples(m, 2, post, 0, 3, 8, 8, autoguidance_scale=float("nan"), guide_model=m)
    with pytest.raises(ValueError, match="exclusive"):
        sampler.get_samples(m, 2, post, 0, 3, 8, 8, autoguidance_scale=1.0, guide_model=m, cfg_scale=0.4, y=[1, 2])


def test_lib_binds_the_autoguided_entry_points():
    assert L.ABI_VERSION == 6
    g = L.dd_autoguidance(None, 1.5)
    assert g.guide is None and g.scale == 1.5
    assert L.dd_autoguidance.guide.offset == 0 and L.dd_autoguidance.scale.offset == C.sizeof(C.c_void_p)
    assert L.SIGNATURES["dd_forward_autoguided"][1][5] == C.POINTER(L.dd_autoguidance)
    for name, args in (("dd_sample_autoguided", L.dd_sample_args), ("dd_sample_affine_autoguided", L.dd_affine_sample_args),
                       ("dd_sample_multistep_autoguided", L.dd_multistep_sample_args)):
        assert L.SIGNATURES[name][1] == [C.c_void_p, C.POINTER(args), C.POINTER(L.dd_autoguidance), C.c_void_p]
    lib = L.load()
    assert lib.dd_abi_version() == 6
    for name in ("dd_forward_autoguided", "dd_sample_autoguided", "dd_sample_affine_autoguided", "dd_sample_multistep_autoguided"):
        assert hasattr(lib, name)


# ---- GPU ------------------------------------------------------------------------------------------------------------------
TINY_G = dict(TINY, depth=1)                                   # the guide: 1 block, embed_dim 64
TINY_M = dict(TINY, depth=3, embed_dim=128, num_heads=2)       # the main model: 3 blocks, embed_dim 128


def _pair(cfg_g, cfg_m, seeds, max_batch, precision="bf16"):
    """(guide, main) engine models"""
    return engine_pair(cfg_g, cfg_m, seeds, max_batch, precision)[:2]


def _tiny_pair(seeds=(41, 42), max_batch=12, precision="bf16"):
    return _pair(TINY_G, TINY_M, seeds, max_batch, precision)


@gpu
@pytest.mark.parametrize("case", ["tiny_one_tile", "tiled_32x32", "conditional_main_unconditional_guide"])
def test_forward_autoguided_vs_oracle(case):
    """dd_forward_autoguided against the numpy oracle's two forwards combined in numpy fp32 in the stated order.
    fp32 engine: |eps - want| <= (1 + 2|s|) 1e-4 (the per-model fp32 bound is 1e-4; worst case (1 + |s|) e_main + |s| e_guide);
    bf16 engine: rms <= ((1 + |s|) bound(depth_main) + |s| bound(depth_guide)) sigma, the existing error model applied to the formula."""
    import oracle
    base = dict(img_size=32, patch_size=2, in_chans=4, mlp_ratio=4, qkv_bias=False, mlp_time_embed=False, num_classes=-1,
                normalize_timesteps=False)
    if case == "tiny_one_tile":
        cfg_g, cfg_m, B, S, Cc = TINY_G, TINY_M, 5, 8, 3
    elif case == "tiled_32x32":
        cfg_g, cfg_m = dict(base, embed_dim=128, depth=1, num_heads=2), dict(base, embed_dim=256, depth=3, num_heads=4)
        B, S, Cc = 4, 32, 4
    else:
        cfg_g, cfg_m, B, S, Cc = dict(TINY_G, mlp_time_embed=True), dict(TINY_M, num_classes=11), 5, 8, 3
    s, t = 1.7, 611.0
    mp_g, mp_m = ModelParams.from_dict(cfg_g), ModelParams.from_dict(cfg_m)
    o_g = oracle.UViTOracle(mp_g.as_dict(), {k: v.numpy() for k, v in synthetic_state_dict(mp_g, 61).items()})
    o_m = oracle.UViTOracle(mp_m.as_dict(), {k: v.numpy() for k, v in synthetic_state_dict(mp_m, 62).items()})
    gen = torch.Generator().manual_seed(63)
    x = torch.randn(B, Cc, S, S, generator=gen)
    y = torch.randint(0, 11, (B,), generator=gen) if mp_m.num_classes > 0 else None
    tv = np.full((B,), t, F32)
    e_m = o_m(x.numpy(), tv, y.numpy() if y is not None else None).astype(F32)
    e_g = o_g(x.numpy(), tv, None).astype(F32)
    d = (e_m - e_g).astype(F32)
    want = (e_m + (F32(s) * d).astype(F32)).astype(F32)
    sigma = float(want.std())
    for prec in ("fp32", "bf16"):
        eg, em = _pair(cfg_g, cfg_m, (61, 62), B, prec)
        got = em.forward_autoguided(x.cuda(), t, y.cuda() if y is not None else None, eg, s).cpu().numpy()
        plain = em.forward_autoguided(x.cuda(), t, y.cuda() if y is not None else None, em, s).cpu().numpy()    # guide == the model: plain forward
        own = em.forward(x.cuda(), t, y.cuda() if y is not None else None).cpu().numpy()
        torch.cuda.synchronize()
        assert np.isfinite(got).all()
        err = float(np.abs(got.astype(np.float64) - want).max())
        rms = float(np.sqrt(((got.astype(np.float64) - want) ** 2).mean()))
        bound = (1 + abs(s)) * eps_rms_bound(mp_m.depth) + abs(s) * eps_rms_bound(mp_g.depth)
        print(f"{case} {prec}: autoguided eps vs oracle max {err:.3e} rms {rms:.3e} (sigma {sigma:.3f}; bf16 bound {bound * sigma:.3e})")
        if prec == "fp32":
            assert err <= (1 + 2 * abs(s)) * 1e-4
        else:
            assert rms <= bound * sigma
        assert np.array_equal(plain, own), "guide == the running model is not the plain forward"
        assert not np.array_equal(got, own)
        del eg, em


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", ["tiny_forced", "celeba_b128"])
def test_scale_zero_equals_the_unguided_loop(case, kind):
    """scale 0 with Philox noise == the unguided loop of the main model, bit for bit, in every loop."""
    if case == "tiny_forced":
        B, S, n, flags = 6, 8, 8, L.DD_DEV_FORCE_CHAINS
        eg, em = _tiny_pair(max_batch=B)
    else:
        B, S, n, flags = 128, 64, 3, 0
        eg, em = celeba_pair(B)[:2]
    ctx, x0, stream = em.ctx, images(B, 3, S, 7), side_stream()
    want = run_first_steps(kind, em, None, x0, stream, switch=0, n=n, seed=21, flags=flags)
    chains = ctx.lib.dd_dev_last_sample_chains(ctx.handle)
    got = run_first_steps(kind, em, None, x0, stream, switch=0, n=n, seed=21, flags=flags, guidance=Autoguidance(eg, 0.0))
    assert chains == ctx.lib.dd_dev_last_sample_chains(ctx.handle) == 2
    assert torch.isfinite(got).all() and not torch.equal(got if kind != "multistep" else got[0], x0)
    assert torch.equal(got, want), "scale 0 differs from the unguided loop"


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_the_guides_identity_decides_the_launch_not_its_weights(kind):
    """guide == the running model, at any scale: the unguided loop's launches (no graph is captured beyond the unguided one) and bits.
    A separately created model with the same weights as guide at s = 1.7 goes through the two-model path (it captures) and is
    byte-identical too: d is exactly 0 and the kernels are deterministic."""
    B = 4
    _, em = _tiny_pair(max_batch=B)
    _, twin = _tiny_pair(max_batch=B)                # the same seeds: the same weights, another dd_model
    ctx, x0, stream = em.ctx, images(B, 3, 8, 9), side_stream()
    want = run_first_steps(kind, em, None, x0, stream, switch=0, seed=22)
    n0 = ctx.lib.dd_dev_graph_captures(ctx.handle)
    same = run_first_steps(kind, em, None, x0, stream, switch=0, seed=22, guidance=Autoguidance(em, 1.7))
    assert ctx.lib.dd_dev_graph_captures(ctx.handle) == n0, "guide == the running model captured a graph of its own"
    other = run_first_steps(kind, em, None, x0, stream, switch=0, seed=22, guidance=Autoguidance(twin, 1.7))
    assert ctx.lib.dd_dev_graph_captures(ctx.handle) == n0 + 1, "the two-model path did not capture its own graph"
    assert torch.isfinite(want).all()
    assert torch.equal(same, want), "guide == the running model differs from the unguided loop"
    assert torch.equal(other, want), "a guide with the same weights (d == 0) differs from the unguided loop"


@gpu
def test_the_duodiff_call():
    """first = guide = shallow, late = full, t_switch = 300, s = 1.7: x after the DDPM steps up to the switch (t_end = 700) is
    byte-identical to dd_sample's; the final x (t_end = 690) differs from the unguided result and equals the manual loop of
    sample_step (shallow) / forward_autoguided + ddpm_step (full) with the same noise."""
    from duodiff_amd.engine import sample_loop
    B, s = 4, 1.7
    eg, em = _tiny_pair(max_batch=B)
    ctx, x0, stream = em.ctx, images(B, 3, 8, 10), side_stream()
    out = {}
    with torch.cuda.stream(stream):
        for name, ag in (("unguided", None), ("auto", Autoguidance(eg, s))):
            for t_end in (700, 690):
                x = x0.clone()
                sample_loop(ctx, eg, em, x, t_switch=300, t_start=999, t_end=t_end, seed=23, noise="philox", stream=stream, guidance=ag)
                stream.synchronize()
                out[name, t_end] = x
        # the manual loop, without noise (Philox z exists inside the fused kernels only)
        xl = x0.clone()
        sample_loop(ctx, eg, em, xl, t_switch=300, t_start=999, t_end=690, noise="none", stream=stream, guidance=Autoguidance(eg, s))
        xm, eps = x0.clone(), torch.empty_like(x0)
        for t in range(999, 689, -1):
            if t >= 700:
                eg.sample_step(xm, t, noise="none", stream=stream)
            else:
                em.forward_autoguided(xm, t, None, eg, s, out=eps, stream=stream)
                ctx.ddpm_step(xm, eps, None, t, out=xm, stream=stream)
        stream.synchronize()
    assert torch.equal(out["auto", 700], out["unguided", 700]), "x up to the switch differs from dd_sample's"
    assert torch.isfinite(out["auto", 690]).all() and not torch.equal(out["auto", 690], out["unguided", 690])
    assert torch.isfinite(xm).all() and torch.equal(xl, xm), "the DuoDiff call differs from the manual loop"


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_autoguided_loops_equal_manual_steps(kind):
    """No noise, s = 1.7, the backbone switch inside (the guide runs the first steps itself): the device loop, graph-replayed and eager,
    == forward_autoguided + ddpm_step / affine_step / multistep_step per step; and (Philox noise) the loop cut at a save point, with
    counter_base and h carried over, == the uncut loop."""
    B, s, n, sw = 4, 1.7, 8, 3
    eg, em = _tiny_pair(max_batch=B)
    x0, stream = images(B, 3, 8, 11), side_stream()
    ag = Autoguidance(eg, s)
    loops = [run_first_steps(kind, eg, em, x0, stream, switch=sw, n=n, noise="none", use_graph=ug, guidance=ag) for ug in (True, False)]
    xm, h = run_steps(kind, eg, x0, first_rows(kind, n), stream, late=em, switch_after=sw, noise="none", guidance=ag)
    manual = xm if kind != "multistep" else torch.stack([xm, h])
    assert torch.isfinite(manual).all() and not torch.equal(xm, x0)
    assert torch.equal(loops[0], loops[1]), "graph replay differs from eager launches"
    assert torch.equal(loops[0], manual), "the autoguided loop differs from its manual steps"
    if kind == "ddpm":
        return
    # save-point cut after 5 steps (past the switch): counter_base = 5, h carried over
    whole = run_first_steps(kind, eg, em, x0, stream, switch=sw, n=n, seed=24, guidance=ag)
    cut = run_first_steps(kind, eg, em, x0, stream, switch=sw, n=n, seed=24, guidance=ag, cuts=(5,))
    assert torch.equal(cut, whole), "the cut loop differs from the uncut loop"


@gpu
@pytest.mark.parametrize("case", ["tiny_forced", "celeba_b128", "imagenet256_b32"])
def test_autoguided_two_chains_equal_one_chain(case):
    """Autoguided DDPM loop, s = 1.7, Philox noise, switch inside: two half-batch chains (each on its chain's workspace of BOTH models)
    == DD_DEV_NO_CHAINS, bit for bit."""
    y = None
    if case == "tiny_forced":
        B, S, Cc, n, sw, force = 6, 8, 3, 8, 3, L.DD_DEV_FORCE_CHAINS
        eg, em = _tiny_pair(max_batch=B)
    elif case == "celeba_b128":
        B, S, Cc, n, sw, force = 128, 64, 3, 3, 1, 0
        eg, em = celeba_pair(B)[:2]
    else:
        B, S, Cc, n, sw, force = 32, 32, 4, 3, 1, 0
        eg, em = imagenet256_pair(B, (53, 54))[:2]
        y = labels(B, 1000, 12)
    ctx, x0, stream = em.ctx, images(B, Cc, S, 12), side_stream()
    outs = {}
    for name, flags in (("chained", force), ("single", L.DD_DEV_NO_CHAINS)):
        x = run_first_steps("ddpm", eg, em, x0, stream, switch=sw, n=n, seed=25, y=y, flags=flags, guidance=Autoguidance(eg, 1.7))
        outs[name] = (x, ctx.lib.dd_dev_last_sample_chains(ctx.handle))
    assert outs["chained"][1] == 2 and outs["single"][1] == 1
    assert torch.isfinite(outs["single"][0]).all() and not torch.equal(outs["single"][0], x0)
    assert torch.equal(outs["chained"][0], outs["single"][0]), "autoguided chains differ from the single chain"


@gpu
def test_no_stale_graph():
    """A new scale, a new guide and swapped roles each re-capture and each equal a run on freshly built models; classifier-free,
    autoguided and unguided calls alternated on one (class-conditional) pair each reproduce their own first result."""
    B = 4
    cfg_g, cfg_m = dict(TINY_G, num_classes=11), dict(TINY_M, num_classes=11)
    x0, stream = images(B, 3, 8, 13), side_stream()
    y = labels(B, 10, 14)

    def models():
        eg, em = _pair(cfg_g, cfg_m, (41, 42), 2 * B)
        g2, _ = uvit(cfg_g, 43, "bf16", 2 * B)
        return eg, em, g2.engine_model(2 * B)

    def run(ms, what):
        eg, em, eg2 = ms
        kw = dict(switch=0, seed=26, y=y)
        return {"s0.4": lambda: run_first_steps("ddpm", em, None, x0, stream, guidance=Autoguidance(eg, 0.4), **kw),
                "s1.7": lambda: run_first_steps("ddpm", em, None, x0, stream, guidance=Autoguidance(eg, 1.7), **kw),
                "guide2": lambda: run_first_steps("ddpm", em, None, x0, stream, guidance=Autoguidance(eg2, 1.7), **kw),
                "swapped": lambda: run_first_steps("ddpm", eg, None, x0, stream, guidance=Autoguidance(em, 1.7), **kw),
                "cfg": lambda: run_first_steps("ddpm", em, None, x0, stream, guidance=(1.7, 10), **kw),
                "plain": lambda: run_first_steps("ddpm", em, None, x0, stream, **kw)}[what]()

    ms = models()
    ctx = ms[0].ctx
    order = ["s0.4", "s1.7", "s0.4", "guide2", "s1.7", "swapped", "cfg", "s1.7", "plain", "cfg", "s1.7", "plain"]
    got, caps = [], []
    for what in order:
        n0 = ctx.lib.dd_dev_graph_captures(ctx.handle)
        got.append(run(ms, what))
        caps.append(ctx.lib.dd_dev_graph_captures(ctx.handle) - n0)
    assert caps == [1] * len(order), caps          # every call here changes scale, guide, roles or guidance form against the call before
    fresh = {}
    for what in set(order):
        f = models()
        fresh[what] = run(f, what)
        del f
    for a in ("s0.4", "s1.7", "guide2", "cfg"):
        assert not torch.equal(fresh[a], fresh["plain"]), a
    assert not torch.equal(fresh["s0.4"], fresh["s1.7"]) and not torch.equal(fresh["guide2"], fresh["s1.7"])
    assert not torch.equal(fresh["cfg"], fresh["s1.7"])
    for what, x in zip(order, got):
        assert torch.equal(x, fresh[what]), f"{what}: replayed a stale graph"


@gpu
def test_autoguided_loop_reads_no_stale_workspace_bytes():
    """Both chains' workspaces of both models poisoned (NaN bytes) in front of the first autoguided dd_sample == fresh models."""
    B = 6
    x0, stream = images(B, 3, 8, 15), side_stream()
    outs = []
    for poison in (False, True):
        eg, em = _tiny_pair(seeds=(71, 72), max_batch=B)
        ctx = em.ctx
        if poison:
            with torch.cuda.stream(stream):
                for e in (eg, em):
                    ctx.check(ctx.lib.dd_dev_poison_workspaces(ctx.handle, e.handle, stream.cuda_stream))
        x = run_first_steps("ddpm", eg, em, x0, stream, switch=3, seed=27, flags=L.DD_DEV_FORCE_CHAINS, guidance=Autoguidance(eg, 1.7))
        outs.append((x, ctx.lib.dd_dev_last_sample_chains(ctx.handle)))
        del eg, em
    assert outs[0][1] == outs[1][1] == 2
    assert torch.isfinite(outs[0][0]).all() and not torch.equal(outs[0][0], x0)
    assert torch.equal(outs[0][0], outs[1][0]), "autoguided loop differs after the workspaces were poisoned"


@gpu
def test_invalid_autoguided_calls_are_rejected_before_anything_is_enqueued():
    """DD_ERR_INVALID with a message, x and eps untouched and no graph captured, for every case of the header's list."""
    from duodiff_amd.engine import Context, Model
    B = 4
    eg, em = _tiny_pair(max_batch=B)
    ctx, lib = em.ctx, em.ctx.lib
    mk = lambda cfg, seed, mb=B: uvit(cfg, seed, "bf16", mb)[0].engine_model(mb)
    g_img, g_patch, g_chan = mk(dict(TINY_G, img_size=16), 81), mk(dict(TINY_G, patch_size=4), 82), mk(dict(TINY_G, in_chans=4), 83)
    g_small, m_small = mk(TINY_G, 84, B - 1), mk(TINY_M, 85, B - 1)
    g_cond, m_cond = mk(dict(TINY_G, num_classes=11), 86), mk(dict(TINY_M, num_classes=11), 87)
    g_raw = Model(ctx, ModelParams.from_dict(TINY_G), B)                      # never finalized
    g_ee = Model(ctx, ModelParams.from_dict(TINY_G), B)
    g_ee.enable_early_exit("mlp_probe_per_layer")
    for k, v in synthetic_state_dict(ModelParams.from_dict(TINY_G), 88).items():
        g_raw.set_param(k, v)
    m_ee = Model(ctx, ModelParams.from_dict(TINY_M), B)
    m_ee.enable_early_exit("mlp_probe_per_layer")
    other_ctx = Context(ctx.device)                                           # a second dd_ctx on the same GPU
    g_other = Model(other_ctx, ModelParams.from_dict(TINY_G), B)
    for k, v in synthetic_state_dict(ModelParams.from_dict(TINY_G), 90).items():
        g_other.set_param(k, v)
    g_other.finalize("bf16")
    x0, stream = images(B, 3, 8, 17), side_stream()
    y = labels(B, 10, 18)
    NULLG = object()
    #        first  late   guide    scale          y     message
    cases = [(em, None, NULLG, 1.0, None, "dd_autoguidance"), (em, None, None, 1.0, None, "guide"),
             (em, None, g_other, 1.0, None, "context"), (em, None, g_raw, 1.0, None, "finalize"),
             (em, None, g_img, 1.0, None, "geometry"), (em, None, g_patch, 1.0, None, "geometry"), (em, None, g_chan, 1.0, None, "geometry"),
             (eg, em, g_patch, 1.0, None, "geometry"),
             (em, None, g_ee, 1.0, None, "early-exit"), (m_ee, None, eg, 1.0, None, "early-exit"),
             (em, None, eg, float("inf"), None, "finite"), (em, None, eg, float("nan"), None, "finite"),
             (em, None, g_small, 1.0, None, "max_batch"), (m_small, None, eg, 1.0, None, "max_batch"),
             (m_cond, None, eg, 1.0, None, "labels"), (em, None, g_cond, 1.0, None, "labels"), (em, None, eg, 1.0, y, "labels"),
             (em, None, eg, 1.0, None, "host noise")]
    n0 = lib.dd_dev_graph_captures(ctx.handle)
    sp = C.c_void_p(stream.cuda_stream)
    for first, late, guide, scale, yy, msg in cases:
        gs = L.dd_autoguidance(guide.handle if guide not in (None, NULLG) else None, scale)
        gp = None if guide is NULLG else C.byref(gs)
        entries = ("sample", "affine", "multistep") if late is not None or msg == "host noise" else ("forward", "sample", "affine", "multistep")
        noise_mode = L.DD_NOISE_BUFFER if msg == "host noise" else L.DD_NOISE_NONE
        for entry in entries:
            x, eps, h = x0.clone(), torch.zeros_like(x0), torch.zeros_like(x0)
            yp = yy.data_ptr() if yy is not None else None
            with torch.cuda.stream(stream):
                if entry == "forward":
                    rc = lib.dd_forward_autoguided(ctx.handle, first.handle, C.c_void_p(x.data_ptr()), 500.0, C.c_void_p(yp), gp,
                                                   C.c_void_p(eps.data_ptr()), B, sp)
                elif entry == "sample":
                    a = L.dd_sample_args()
                    a.first, a.late, a.t_switch, a.t_start, a.t_end = first.handle, late.handle if late else None, 3, 999, 995
                    a.noise_mode, a.use_graph, a.seed, a.y_dev, a.x_dev, a.B = noise_mode, 1, 1, yp, x.data_ptr(), B
                    rc = lib.dd_sample_autoguided(ctx.handle, C.byref(a), gp, sp)
                else:
                    n = 3
                    f, one, nz = (C.c_float * n)(900.0, 600.0, 300.0), (C.c_float * n)(1.0, 1.0, 1.0), (C.c_int32 * n)(0, 0, 0)
                    a = L.dd_affine_sample_args() if entry == "affine" else L.dd_multistep_sample_args()
                    a.first, a.late, a.n_steps, a.switch_after = first.handle, late.handle if late else None, n, 1
                    a.t, a.a, a.b, a.c, a.noise = f, one, one, one, nz
                    a.noise_mode, a.use_graph, a.seed, a.y_dev, a.x_dev, a.B = noise_mode, 1, 1, yp, x.data_ptr(), B
                    if entry == "affine":
                        rc = lib.dd_sample_affine_autoguided(ctx.handle, C.byref(a), gp, sp)
                    else:
                        a.d, a.p, a.q, a.hist, a.h_dev = one, one, one, nz, h.data_ptr()
                        rc = lib.dd_sample_multistep_autoguided(ctx.handle, C.byref(a), gp, sp)
            stream.synchronize()
            err = lib.dd_last_error(ctx.handle).decode()
            assert rc == L.DD_ERR_INVALID, f"{entry} {msg}: status {rc} ({err})"
            assert (msg in err) or (msg == "host noise" and "noise" in err), f"{entry} {msg}: {err!r}"
            assert torch.equal(x, x0) and not eps.any() and not h.any(), f"{entry} {msg}: something was enqueued"
    assert lib.dd_dev_graph_captures(ctx.handle) == n0
    with pytest.raises(ValueError):
        em.forward_autoguided(x0, 500.0, None, g_img, 1.0)


@gpu
def test_cli_autoguided_end_to_end(tmp_path):
    """The DuoDiff command line with --autoguidance_scale in fp32 with the torch CPU noise stream, against the oracle's rollout whose
    model output is the two oracles' eps combined in numpy fp32 while the full model runs (test_cli_end_to_end's tolerance)."""
    import oracle
    import yaml
    cfg_s, cfg_f, s = dict(TINY_G, img_size=16), dict(TINY_M, img_size=16), 0.8
    orc = {}
    for name, cfg, seed in (("s", cfg_s, 1), ("f", cfg_f, 2)):
        (tmp_path / f"{name}.yaml").write_text(yaml.safe_dump({"model_params": cfg}))
        mp = ModelParams.from_dict(cfg)
        sd = synthetic_state_dict(mp, seed)
        torch.save(dict(sd), tmp_path / f"{name}.pth")
        orc[name] = oracle.UViTOracle(mp.as_dict(), {k: v.numpy() for k, v in sd.items()})
    out = tmp_path / "out"
    cmd = [sys.executable, "-m", "duodiff_amd.sampler", "--seed", "4", "--checkpoint_path", str(tmp_path / "s.pth"),
           "--checkpoint_path_late", str(tmp_path / "f.pth"), "--config_path", str(tmp_path / "s.yaml"),
           "--config_path_late", str(tmp_path / "f.yaml"), "--t_switch", "300", "--batch_size", "3",
           "--parametrization", "predict_noise", "--output_folder", str(out), "--no_png", "--precision", "fp32",
           "--noise", "torch_cpu", "--autoguidance_scale", str(s)]
    r = subprocess.run(cmd, cwd=str(REPO), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out / "samples.npy")
    assert got.shape == (3, 16, 16, 3) and got.dtype == np.float32 and np.isfinite(got).all()

    def guided_full(x, t, y):
        e_m, e_g = orc["f"](x, t, y).astype(F32), orc["s"](x, t, y).astype(F32)
        return (e_m + (F32(s) * (e_m - e_g).astype(F32)).astype(F32)).astype(F32)

    want, _ = oracle.get_samples(orc["s"], 3, 4, 3, 16, 16, late_model=guided_full, t_switch=300)
    plain, _ = oracle.get_samples(orc["s"], 3, 4, 3, 16, 16, late_model=orc["f"], t_switch=300)
    scale = max(1.0, float(np.abs(want).max()))
    print(f"CLI autoguided vs oracle rollout: max abs {np.abs(got - want).max():.3e} (tolerance {5e-3 * scale:.3e}; "
          f"unguided rollout differs by {np.abs(plain - want).max():.3e})")
    assert np.abs(plain - want).max() > 5e-3 * scale                         # the guidance is visible at this tolerance
    np.testing.assert_allclose(got, want, rtol=0, atol=5e-3 * scale)
