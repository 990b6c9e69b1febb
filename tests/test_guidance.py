"""Classifier-free guidance: eps = eps_c + s (eps_c - eps_u) fused into the step kernels (dd_forward_guided, dd_sample_guided,
dd_sample_affine_guided) and the sampler options --cfg_scale / --cfg_null_label / --class_label.

CPU tests: the command line and the ctypes binding.  GPU tests (marked): the guided eps against the numpy oracle run twice, the
loops against their own building blocks bit for bit, chains, graph keys, stale workspace bytes, argument errors, the CLI.
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
from loop_support import NULL, TINY_COND, cli_argv, ddpm_rows, engine_pair, eps_rms_bound, imagenet256_pair, images, labels, run_loop
from loop_support import run_steps, side_stream, uvit

gpu = pytest.mark.gpu

IMAGENET256 = REPO / "configs" / "uvit_imagenet256.yaml"
IMAGENET256_3 = REPO / "configs" / "uvit_imagenet256_3.yaml"


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_cli_guidance_options_and_defaults():
    from duodiff_amd import sampler
    a = sampler.get_args(cli_argv(IMAGENET256))
    assert a.cfg_scale is None and a.cfg_null_label == 1000 and a.class_label is None and a.class_id is None
    a = sampler.get_args(cli_argv(IMAGENET256, "--cfg_scale", "0.4", "--class_label", "207", "--cfg_null_label", "999"))
    assert a.cfg_scale == pytest.approx(0.4) and a.class_label == 207 and a.cfg_null_label == 999
    a = sampler.get_args(cli_argv(IMAGENET256, "--cfg_scale", "0"))
    assert a.cfg_scale == 0.0 and a.cfg_scale is not None       # 0 selects the guided path too
    y = sampler.labels_from_args(sampler.get_args(cli_argv(IMAGENET256, "--class_label", "207")), 3, 1001)
    assert y.dtype == torch.int64 and y.tolist() == [207, 207, 207]
    assert sampler.labels_from_args(sampler.get_args(cli_argv(IMAGENET256)), 3, 1001) is None


@pytest.mark.parametrize("config,extra,match", [
    ("uvit_celeba.yaml", ["--cfg_scale", "0.4", "--class_id", "3"], "class-conditional"),        # unconditional config
    ("uvit_imagenet64.yaml", ["--cfg_scale", "0.4", "--class_label", "3"], "null"),             # num_classes 1000: no null row
    ("uvit_imagenet256.yaml", ["--cfg_scale", "0.4"], "labels"),                                  # guidance without labels
    ("uvit_imagenet256.yaml", ["--class_label", "1001"], "class_label"),                         # label outside [0, num_classes)
    ("uvit_imagenet256.yaml", ["--class_label", "-1"], "class_label"),
    ("uvit_celeba.yaml", ["--class_label", "3"], "class-conditional"),
    ("uvit_imagenet256.yaml", ["--cfg_scale", "0.4", "--class_label", "3", "--cfg_null_label", "1001"], "null"),
    ("uvit_imagenet256.yaml", ["--cfg_scale", "nan", "--class_label", "3"], "finite"),
])
def test_cli_rejects_invalid_guidance_before_any_gpu_work(tmp_path, config, extra, match):
    """main() validates the options against the YAML before it builds a model: no GPU is touched (this runs on the CPU box)."""
    from duodiff_amd import sampler
    argv = cli_argv(REPO / "configs" / config, *extra)
    argv[argv.index("--output_folder") + 1] = str(tmp_path / "out")
    with pytest.raises(ValueError, match=match):
        sampler.main(argv)


def test_cli_rejects_a_late_config_without_the_null_row(tmp_path):
    from duodiff_amd import sampler
    argv = cli_argv(IMAGENET256_3, "--cfg_scale", "0.4", "--class_label", "3", "--checkpoint_path_late", "/nonexistent.pth",
                 "--config_path_late", str(REPO / "configs" / "uvit_imagenet64.yaml"), "--output_folder", str(tmp_path / "out"))
    with pytest.raises(ValueError, match="null"):
        sampler.main(argv)


def test_lib_binds_the_guided_entry_points():
    assert L.ABI_VERSION == 6
    assert C.sizeof(L.dd_guidance) == 8
    g = L.dd_guidance(0.4, 1000)
    assert g.null_label == 1000 and abs(g.scale - 0.4) < 1e-7
    assert L.SIGNATURES["dd_forward_guided"][1][5] == C.POINTER(L.dd_guidance)
    assert L.SIGNATURES["dd_sample_guided"][1] == [C.c_void_p, C.POINTER(L.dd_sample_args), C.POINTER(L.dd_guidance), C.c_void_p]
    assert L.SIGNATURES["dd_sample_affine_guided"][1] == [C.c_void_p, C.POINTER(L.dd_affine_sample_args), C.POINTER(L.dd_guidance),
                                                          C.c_void_p]
    lib = L.load()
    assert lib.dd_abi_version() == 6
    for name in ("dd_forward_guided", "dd_sample_guided", "dd_sample_affine_guided"):
        assert hasattr(lib, name)


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def _tiny_pair(seeds=(41, 42), max_batch=12, precision="bf16"):
    return engine_pair(dict(TINY_COND, depth=1), dict(TINY_COND, depth=3), seeds, max_batch, precision)


@gpu
@pytest.mark.parametrize("case", ["tiny_one_tile", "tiled_32x32"])
def test_forward_guided_vs_oracle(case):
    """dd_forward_guided against the unchanged numpy oracle run twice (labels, then the null label), combined in float64."""
    import oracle
    if case == "tiny_one_tile":
        cfg, B, S, Cc = dict(TINY_COND), 5, 8, 3
    else:
        cfg = dict(img_size=32, patch_size=2, in_chans=4, embed_dim=256, depth=3, num_heads=4, mlp_ratio=4, qkv_bias=False,
                   mlp_time_embed=False, num_classes=11, normalize_timesteps=False)
        B, S, Cc = 4, 32, 4
    s, t = 0.4, 611.0
    mp = ModelParams.from_dict(cfg)
    orc = oracle.UViTOracle(mp.as_dict(), {k: v.numpy() for k, v in synthetic_state_dict(mp, 61).items()})
    g = torch.Generator().manual_seed(62)
    x = torch.randn(B, Cc, S, S, generator=g)
    y = torch.randint(0, NULL, (B,), generator=g)
    tv = np.full((B,), t, np.float32)
    ec = orc(x.numpy(), tv, y.numpy()).astype(np.float64)
    eu = orc(x.numpy(), tv, np.full((B,), NULL, np.int64)).astype(np.float64)
    want = ec + s * (ec - eu)
    sigma = float(ec.std())
    for prec in ("fp32", "bf16"):
        m, _ = uvit(cfg, 61, prec, max_batch=2 * B)
        em = m.engine_model(2 * B)
        got = em.forward_guided(x.cuda(), t, y.cuda(), s, NULL).cpu().numpy().astype(np.float64)
        torch.cuda.synchronize()
        assert np.isfinite(got).all()
        err, rms = float(np.abs(got - want).max()), float(np.sqrt(((got - want) ** 2).mean()))
        print(f"{case} {prec}: guided eps vs oracle max {err:.3e} rms {rms:.3e} (sigma {sigma:.3f})")
        if prec == "fp32":
            assert err <= 1e-4
        else:
            assert rms <= eps_rms_bound(mp.depth) * (1 + 2 * s) * sigma
        del em, m


@gpu
@pytest.mark.parametrize("case", ["tiny_forced", "imagenet256_default"])
def test_scale_zero_equals_the_unguided_loop(case):
    """dd_sample_guided with scale 0 and Philox noise == dd_sample with the same labels, bit for bit, backbone switch included."""
    if case == "tiny_forced":
        B, S, Cc, steps, tsw, flags = 6, 8, 3, 10, 4, L.DD_DEV_FORCE_CHAINS
        es, ef, mp = _tiny_pair(max_batch=2 * B)
    else:
        B, S, Cc, steps, tsw, flags = 32, 32, 4, 3, 1, 0
        es, ef, mp = imagenet256_pair(2 * B, (51, 52))
    x0, y, stream = images(B, Cc, S, 7), labels(B, 10, 8), side_stream()
    outs = {}
    for name, guidance in (("unguided", None), ("scale0", (0.0, NULL if case == "tiny_forced" else 1000))):
        outs[name] = run_loop("ddpm", es, x0, ddpm_rows(steps), stream, late=ef, t_switch=tsw, y=y, seed=21, flags=flags, guidance=guidance)[::2]
    assert outs["unguided"][1] == outs["scale0"][1] == 2
    assert torch.isfinite(outs["scale0"][0]).all() and not torch.equal(outs["scale0"][0], x0)
    assert torch.equal(outs["scale0"][0], outs["unguided"][0]), "scale 0 differs from the unguided loop"


@gpu
def test_guided_loops_equal_manual_steps():
    """Scale 0.4, no noise: dd_sample_guided (graph replay and eager) == forward_guided + ddpm_step per step, and
    dd_sample_affine_guided (DDIM-10) == forward_guided + affine_step per step, bit for bit, backbone switch inside."""
    from duodiff_amd import sampler
    B, s = 4, 0.4
    es, ef, _ = _tiny_pair(max_batch=2 * B)
    x0, y, stream = images(B, 3, 8, 9), labels(B, 10, 10), side_stream()
    kw = dict(late=ef, noise="none", guidance=(s, NULL), y=y)
    rows = ddpm_rows(12)
    loops = [run_loop("ddpm", es, x0, rows, stream, t_switch=5, use_graph=use_graph, **kw)[0] for use_graph in (True, False)]
    xm, _ = run_steps("ddpm", es, x0, rows, stream, switch_after=5, **kw)
    assert torch.equal(loops[0], loops[1]), "graph replay differs from eager launches"
    assert torch.equal(loops[0], xm), "guided DDPM loop differs from forward_guided + ddpm_step"
    assert torch.isfinite(xm).all()

    ts = np.linspace(0, 999, 11).astype(int)[::-1]
    pairs = [(int(a), int(b)) for a, b in zip(ts[:-1], ts[1:])]
    coefs = [sampler.affine_coefficients("ddim", t, t2, 0.0) for t, t2 in pairs]
    rows = dict(t=[float(t) for t, _ in pairs], a=[c[0] for c in coefs], b=[c[1] for c in coefs], c=[c[2] for c in coefs],
                noise=[int(t2 > 0) for _, t2 in pairs])
    xm, _ = run_steps("affine", es, x0, rows, stream, switch_after=4, **kw)
    for use_graph in (True, False):
        xa = run_loop("affine", es, x0, rows, stream, switch_after=4, use_graph=use_graph, **kw)[0]
        assert torch.isfinite(xa).all() and not torch.equal(xa, x0)
        assert torch.equal(xa, xm), f"guided DDIM loop (graph={use_graph}) differs from forward_guided + affine_step"


@gpu
@pytest.mark.parametrize("case", ["tiny_forced", "imagenet256_default"])
def test_guided_two_chains_equal_one_chain(case):
    """Guided loop, scale 0.4, Philox noise, switch inside: the two image-split chains == DD_DEV_NO_CHAINS bit for bit."""
    if case == "tiny_forced":
        B, S, Cc, steps, tsw, force, null = 6, 8, 3, 10, 4, L.DD_DEV_FORCE_CHAINS, NULL
        es, ef, _ = _tiny_pair(max_batch=2 * B)
    else:
        B, S, Cc, steps, tsw, force, null = 32, 32, 4, 3, 1, 0, 1000
        es, ef, _ = imagenet256_pair(2 * B, (51, 52))
    x0, y, stream = images(B, Cc, S, 11), labels(B, 10, 12), side_stream()
    outs = {}
    for name, flags in (("chained", force), ("single", L.DD_DEV_NO_CHAINS)):
        outs[name] = run_loop("ddpm", es, x0, ddpm_rows(steps), stream, late=ef, t_switch=tsw, y=y, seed=23, flags=flags, guidance=(0.4, null))[::2]
    assert outs["chained"][1] == 2 and outs["single"][1] == 1
    assert torch.isfinite(outs["single"][0]).all() and not torch.equal(outs["single"][0], x0)
    assert torch.equal(outs["chained"][0], outs["single"][0]), "guided chains differ from the single chain"


@gpu
def test_a_new_scale_is_not_a_stale_graph():
    """Guided calls at 0.4, 1.0, 0.4 on the same models: each equals a run of freshly built models at that scale."""
    B = 4
    x0, y, stream = images(B, 3, 8, 13), labels(B, 10, 14), side_stream()

    def run(es, ef, scale):
        return run_loop("ddpm", es, x0, ddpm_rows(8), stream, late=ef, t_switch=3, y=y, seed=25, guidance=(scale, NULL))[0]

    es, ef, _ = _tiny_pair(max_batch=2 * B)
    got = [run(es, ef, s) for s in (0.4, 1.0, 0.4)]
    fresh = {}
    for s in (0.4, 1.0):
        fs, ff, _ = _tiny_pair(max_batch=2 * B)
        fresh[s] = run(fs, ff, s)
        del fs, ff
    assert not torch.equal(fresh[0.4], fresh[1.0])
    for s, g in zip((0.4, 1.0, 0.4), got):
        assert torch.equal(g, fresh[s]), f"scale {s}: replayed a graph of another scale"


@gpu
def test_guided_loop_reads_no_stale_workspace_bytes():
    """One guided tiny case with both chains' workspaces poisoned (NaN bytes) before the call == the same case on fresh models."""
    B = 6
    x0, y, stream = images(B, 3, 8, 15), labels(B, 10, 16), side_stream()
    outs = []
    for poison in (False, True):
        es, ef, _ = _tiny_pair(seeds=(71, 72), max_batch=2 * B)
        ctx = es.ctx
        if poison:
            with torch.cuda.stream(stream):
                for e in (es, ef):
                    ctx.check(ctx.lib.dd_dev_poison_workspaces(ctx.handle, e.handle, stream.cuda_stream))
        outs.append(run_loop("ddpm", es, x0, ddpm_rows(8), stream, late=ef, t_switch=3, y=y, seed=27, flags=L.DD_DEV_FORCE_CHAINS,
                             guidance=(0.4, NULL))[::2])
        del es, ef
    assert outs[0][1] == outs[1][1] == 2
    assert torch.isfinite(outs[0][0]).all() and not torch.equal(outs[0][0], x0)
    assert torch.equal(outs[0][0], outs[1][0]), "guided loop differs after the workspaces were poisoned"


@gpu
def test_invalid_guided_calls_are_rejected_before_anything_is_enqueued():
    """DD_ERR_INVALID with a message, the tensors untouched and no graph captured: unconditional model, null label outside
    [0, num_classes) (of either model), 2 B > max_batch, an early-exit model, a non-finite scale."""
    from duodiff_amd.engine import Model, guidance_struct
    B = 4
    es, ef, _ = _tiny_pair(max_batch=2 * B)
    ctx, lib = es.ctx, es.ctx.lib
    small, _ = uvit(dict(TINY_COND, depth=1), 81, "bf16", max_batch=B)          # room for B rows only
    es_small = small.engine_model(B)
    late10, _ = uvit(dict(TINY, depth=1, num_classes=10), 82, "bf16", 2 * B)   # no row for label 10
    el10 = late10.engine_model(2 * B)
    unc, _ = uvit(dict(TINY, depth=1), 83, "bf16", 2 * B)
    eu = unc.engine_model(2 * B)
    ee = Model(ctx, ModelParams.from_dict(TINY_COND), 2 * B)
    ee.enable_early_exit("mlp_probe_per_layer")
    x0 = images(B, 3, 8, 17)
    y = labels(B, 10, 18)
    stream = side_stream()
    cases = [(es, None, (0.4, 11), "null_label"), (es, None, (0.4, -1), "null_label"), (es, el10, (0.4, NULL), "null_label"),
             (eu, None, (0.4, 0), "class-conditional"), (es_small, None, (0.4, NULL), "max_batch"), (ee, None, (0.4, NULL), "early-exit"),
             (es, None, (float("inf"), NULL), "finite")]
    n0 = lib.dd_dev_graph_captures(ctx.handle)
    for first, late, g, msg in cases:
        gs = guidance_struct(g)
        for entry in ("sample", "affine") if late else ("forward", "sample", "affine"):    # (dd_forward_guided has no late model)
            x, eps = x0.clone(), torch.zeros_like(x0)
            with torch.cuda.stream(stream):
                if entry == "forward":
                    rc = lib.dd_forward_guided(ctx.handle, first.handle, C.c_void_p(x.data_ptr()), 500.0, C.c_void_p(y.data_ptr()),
                                               C.byref(gs), C.c_void_p(eps.data_ptr()), B, C.c_void_p(stream.cuda_stream))
                elif entry == "sample":
                    a = L.dd_sample_args()
                    a.first, a.late, a.t_switch, a.t_start, a.t_end = first.handle, late.handle if late else None, 3, 999, 995
                    a.noise_mode, a.use_graph, a.seed, a.y_dev, a.x_dev, a.B = L.DD_NOISE_PHILOX, 1, 1, y.data_ptr(), x.data_ptr(), B
                    rc = lib.dd_sample_guided(ctx.handle, C.byref(a), C.byref(gs), C.c_void_p(stream.cuda_stream))
                else:
                    n = 3
                    f = (C.c_float * n)(900.0, 600.0, 300.0)
                    one = (C.c_float * n)(1.0, 1.0, 1.0)
                    nz = (C.c_int32 * n)(0, 0, 0)
                    a = L.dd_affine_sample_args()
                    a.first, a.late, a.n_steps, a.switch_after = first.handle, late.handle if late else None, n, 1
                    a.t, a.a, a.b, a.c, a.noise = f, one, one, one, nz
                    a.noise_mode, a.use_graph, a.seed, a.y_dev, a.x_dev, a.B = L.DD_NOISE_NONE, 1, 1, y.data_ptr(), x.data_ptr(), B
                    rc = lib.dd_sample_affine_guided(ctx.handle, C.byref(a), C.byref(gs), C.c_void_p(stream.cuda_stream))
            stream.synchronize()
            assert rc == L.DD_ERR_INVALID, f"{entry} {msg}: status {rc}"
            assert msg in lib.dd_last_error(ctx.handle).decode(), lib.dd_last_error(ctx.handle).decode()
            assert torch.equal(x, x0) and not eps.any(), f"{entry} {msg}: something was enqueued"
    assert lib.dd_dev_graph_captures(ctx.handle) == n0
    with pytest.raises(ValueError):
        es.forward_guided(x0, 500.0, y, 0.4, 11)


@gpu
def test_cli_guided_end_to_end(tmp_path):
    """A synthetic class-conditional checkpoint with U-ViT's null row (num_classes 1001): --cfg_scale 0.4 --class_label 3 writes
    finite samples of the right shape, which differ from the --cfg_scale 0 run."""
    import yaml
    cfg = dict(TINY, depth=3, img_size=16, num_classes=1001)
    (tmp_path / "m.yaml").write_text(yaml.safe_dump({"model_params": cfg}))
    torch.save(dict(synthetic_state_dict(ModelParams.from_dict(cfg), 91)), tmp_path / "m.pth")
    got = {}
    for scale in ("0.4", "0"):
        out = tmp_path / f"out{scale}"
        cmd = [sys.executable, "-m", "duodiff_amd.sampler", "--seed", "5", "--checkpoint_path", str(tmp_path / "m.pth"),
               "--config_path", str(tmp_path / "m.yaml"), "--batch_size", "3", "--parametrization", "predict_noise",
               "--output_folder", str(out), "--no_png", "--cfg_scale", scale, "--class_label", "3"]
        r = subprocess.run(cmd, cwd=str(REPO), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        got[scale] = np.load(out / "samples.npy")
        assert got[scale].shape == (3, 16, 16, 3) and np.isfinite(got[scale]).all()
    assert not np.array_equal(got["0.4"], got["0"])
