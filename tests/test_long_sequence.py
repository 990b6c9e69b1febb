"""Whole-model tests of sequences longer than 288 tokens (csrc/attention.hip attention_long_kernel behind the head-major qkv Linear; every other
stage of the forward is the one the short models run): synthetic 3-block models against the numpy oracle (oracle.UViTOracle, pinned to the
reference by tests/test_oracle_golden.py), both engines, with the bounds of tests/test_gpu_parity.py's oracle tests -- fp32: max |eps - ref| <=
1e-4; bf16: rms <= eps_rms_bound(depth) sigma (loop_support: the error model of the bf16 engine).  The configurations put the long sequence
through each family of launches: embed_dim 128 (fused block tail with the next qkv inside, N = 324 not a multiple of 16 or 32), 512
class-conditional (fused tail, two extra tokens), 768 (row-resident Linears, N % 32 == 0), 1024 (GEMM path, 4 latent channels at patch 2) and
one 1024-patch model; a sixth, embed_dim 1024 at 1024 patches, is the family that runs split-K.  Then, without a tolerance: a forward after
dd_dev_poison_workspaces equals a forward on a fresh model bit for bit, in every configuration and both engines (with NaN in the rows [L, Lp)
of every head-major qkv unit: no kernel reads them); an image does not depend on its batch, the first and the last image of every family;
the device loops replay a graph on two half-batch chains bit-identically to the eager single chain; what keeps a bound is refused where it is
set up, with nothing launched.  The launches themselves are gated per element by tests/test_long_geometry.py."""
import numpy as np
import pytest
import torch

import oracle
from duodiff_amd.config import ModelParams
from duodiff_amd.weights import synthetic_state_dict
from loop_support import dev_flags, eps_rms_bound, images, side_stream, uvit

pytestmark = pytest.mark.gpu

FP32_MAX_ERR = 1e-4          # the fp32 bound of tests/test_gpu_parity.py's oracle tests


def cfg(embed_dim, img, patch=4, in_chans=3, num_classes=-1):
    return dict(img_size=img, patch_size=patch, in_chans=in_chans, embed_dim=embed_dim, depth=3, num_heads=embed_dim // 64, mlp_ratio=4,
                qkv_bias=False, mlp_time_embed=False, num_classes=num_classes, normalize_timesteps=True)


L325 = cfg(128, 72)          # 324 patches + the time token


def inputs(c, B, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, c["in_chans"], c["img_size"], c["img_size"], generator=g)
    y = torch.randint(0, c["num_classes"], (B,), generator=g) if c["num_classes"] > 0 else None
    return x, torch.full((B,), 417.0), y


def test_a_325_token_model_loads_and_runs():
    """model creation refused every sequence above 288 tokens before the streaming attention kernel"""
    m, _ = uvit(L325, 11, "bf16", max_batch=2)
    x, t, _ = inputs(L325, 2, 1)
    got = m(x, t, None).cpu().numpy()
    assert got.shape == (2, 3, 72, 72) and np.isfinite(got).all() and got.std() > 0


# the five configurations every whole-model test below shares: (name, config, batch)
CONFIGS = [
    ("D128 L325", L325, 3),
    ("D512 L578 class-conditional", cfg(512, 96, num_classes=10), 2),
    ("D768 L577", cfg(768, 96), 2),
    ("D1024 L577 latents", cfg(1024, 48, patch=2, in_chans=4), 2),
    ("D128 L1025", cfg(128, 128), 1),
]
CONFIG_IDS = ["d128_l325", "d512_l578", "d768_l577", "d1024_l577", "d128_l1025"]


@pytest.mark.parametrize("name,c,B", CONFIGS, ids=CONFIG_IDS)
def test_long_sequence_models_vs_oracle(name, c, B):
    x, t, y = inputs(c, B, 77 + B)
    mp = ModelParams.from_dict(c)
    ref = oracle.UViTOracle(mp.as_dict(), {k: v.numpy() for k, v in synthetic_state_dict(mp, 4245).items()})
    want = ref(x.numpy(), t.numpy(), y.numpy() if y is not None else None)
    sigma = float(want.std())
    for prec in ("fp32", "bf16"):
        m, _ = uvit(c, 4245, prec, max_batch=B)
        got = m(x, t, y).cpu().numpy()
        del m
        assert np.isfinite(got).all()
        err, rms = float(np.abs(got - want).max()), float(np.sqrt(((got - want).astype(np.float64) ** 2).mean()))
        print(f"{name} B={B} {prec}: vs oracle max {err:.3e} rms {rms:.3e} = {rms / sigma:.3e} sigma (sigma {sigma:.3f}; "
              f"bounds: fp32 max {FP32_MAX_ERR}, bf16 rms {eps_rms_bound(mp.depth):.3e} sigma)")
        if prec == "fp32":
            assert err <= FP32_MAX_ERR
        else:
            assert rms <= eps_rms_bound(mp.depth) * sigma


def test_the_split_k_model_vs_oracle():
    """embed_dim 1024 at 1024 patches (64 x 64 latents, patch 2): the one long family whose N = embed_dim Linears run split-K + reduce_ln.
    choose_paths asks for a row partition of the 256 x 256 kernel at every batch: 1025 B = 256 x 4 B + B has one (one tail row per tile), while
    577 and 1154 rows have none, so the 577-token model above runs the GEMM sequence.  Same bounds as above."""
    test_long_sequence_models_vs_oracle("D1024 L1025 latents (split-K)", cfg(1024, 64, patch=2, in_chans=4), 2)


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_an_image_does_not_depend_on_its_batch(prec):
    m, _ = uvit(L325, 12, prec, max_batch=3)
    x, t, _ = inputs(L325, 3, 2)
    whole = m(x, t, None).cpu().numpy()
    alone = m(x[:1].contiguous(), t[:1], None).cpu().numpy()
    assert np.isfinite(whole).all() and np.array_equal(whole[:1], alone)


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("name,c,B", CONFIGS, ids=CONFIG_IDS)
def test_poisoned_workspaces_do_not_reach_the_output(name, c, B, prec):
    """a forward on a fresh model and a forward after dd_dev_poison_workspaces (every activation buffer 0xFF bytes, on the launch stream; the
    method of tools/poison_probe.py): both finite, bit-identical.  The rows [L, Lp) of every head-major qkv unit then hold NaN where a fresh
    workspace holds zeros: no kernel reads them, nor a stale slab or a padding row"""
    x, t, y = inputs(c, B, 55 + B)
    outs = []
    for poison in (False, True):
        m, _ = uvit(c, 4246, prec, max_batch=B)
        em = m.engine_model(B)
        if poison:
            em.ctx.check(em.ctx.lib.dd_dev_poison_workspaces(em.ctx.handle, em.handle, torch.cuda.current_stream().cuda_stream))
        outs.append(m(x, t, y).cpu().numpy())
        del em, m
    assert np.isfinite(outs[0]).all() and outs[0].std() > 0, f"{name} {prec}: the fresh model's output"
    assert np.isfinite(outs[1]).all(), f"{name} {prec}: NaN after the workspaces were poisoned"
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), f"{name} {prec}: the output depends on what a workspace held"


# bf16 for the four families the test above does not run; fp32 for one of them (the class-conditional one: two extra tokens)
@pytest.mark.parametrize("k,prec", [(1, "bf16"), (2, "bf16"), (3, "bf16"), (4, "bf16"), (1, "fp32")],
                         ids=[CONFIG_IDS[1], CONFIG_IDS[2], CONFIG_IDS[3], CONFIG_IDS[4], CONFIG_IDS[1] + "_fp32"])
def test_first_and_last_image_do_not_depend_on_their_batch(k, prec):
    """the other families: the first and the last image of a batch of 2 (3 at embed_dim 128, L = 1025) equal that image run alone, bit for bit"""
    name, c, B = CONFIGS[k]
    B = max(B, 2) if k != 4 else 3
    m, _ = uvit(c, 12 + k, prec, max_batch=B)
    x, t, y = inputs(c, B, 2 + k)
    whole = m(x, t, y).cpu().numpy()
    assert np.isfinite(whole).all() and whole.std() > 0
    for b in (0, B - 1):
        alone = m(x[b:b + 1].contiguous(), t[b:b + 1], y[b:b + 1].contiguous() if y is not None else None).cpu().numpy()
        assert np.array_equal(whole[b:b + 1].view(np.uint32), alone.view(np.uint32)), f"{name} {prec}: image {b} of {B} differs from the image alone"


def test_device_loops_chained_graph_replay_equals_the_eager_single_chain():
    """4 steps of dd_sample (DDPM, backbone switch inside) and of the table-driven DDIM loop at L = 325: graph replay on two half-batch chains
    against eager launches on one chain, bit for bit (the setup of test_gpu_parity's chain-equality tests).  The DDIM run is the deterministic
    one, eta = 0: at a stride of 250 timesteps the reference's formula for eta > 0 takes the square root of a negative number in its last rows
    (the NaN quirk of DESIGN section 2), and a table of NaN compares nothing; dd_sample's four steps draw the device noise."""
    from duodiff_amd import _lib as L
    from duodiff_amd import sampler
    from duodiff_amd.engine import sample_loop
    B = 4
    m_s, _ = uvit(dict(L325, depth=1), 31, "bf16", max_batch=B)
    m_f, _ = uvit(L325, 32, "bf16", max_batch=B)
    es, ef = m_s.engine_model(B), m_f.engine_model(B)
    ctx = es.ctx
    x0 = images(B, 3, 72, 4)
    stream = side_stream()
    ddpm, ddim = [], []
    for flags, graph in ((L.DD_DEV_FORCE_CHAINS, True), (L.DD_DEV_NO_CHAINS, False)):
        with dev_flags(ctx, flags):
            x = x0.clone()
            with torch.cuda.stream(stream):
                sample_loop(ctx, es, ef, x, t_switch=997, t_start=999, t_end=996, seed=9, noise="philox", use_graph=graph, stream=stream)
            stream.synchronize()
            ddpm.append((x.clone(), ctx.lib.dd_dev_last_sample_chains(ctx.handle)))
            g, _ = sampler.get_samples(m_s, B, sampler.predict_noise_postprocessing, 5, 3, 72, 72, late_model=m_f, noise="device",
                                       use_ddim=True, ddim_steps=4, ddim_eta=0.0, t_switch=400, use_graph=graph)
            ddim.append((g, ctx.lib.dd_dev_last_sample_chains(ctx.handle)))
    for name, (a, b) in (("dd_sample", ddpm), ("DDIM", ddim)):
        assert a[1] == 2 and b[1] == 1, (name, a[1], b[1])
    assert torch.isfinite(ddpm[1][0]).all() and not torch.equal(ddpm[1][0], x0)
    assert torch.equal(ddpm[0][0], ddpm[1][0]), "dd_sample: graph replay on two chains differs from the eager single chain"
    assert np.isfinite(ddim[1][0]).all() and np.array_equal(ddim[0][0], ddim[1][0]), "DDIM: graph replay on two chains differs"


def test_what_keeps_a_bound_is_refused_where_it_is_set_up():
    """perturbed-attention guidance on a 325-token model (its identity launch keeps L <= 288): an error, the output untouched, no graph captured;
    a model above 4096 patches, and a max_batch of 1025-token images beyond the head-major row map: refused at creation"""
    m, _ = uvit(L325, 13, "bf16", max_batch=2)
    em = m.engine_model(2)
    ctx = em.ctx
    x, _, _ = inputs(L325, 1, 3)
    x = x.cuda()
    out = torch.full_like(x, 7.0)
    n0 = ctx.lib.dd_dev_graph_captures(ctx.handle)
    with pytest.raises(NotImplementedError, match="288"):
        em.forward_perturbed(x, 500.0, None, 0.4, [1], out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and ctx.lib.dd_dev_graph_captures(ctx.handle) == n0
    with pytest.raises(NotImplementedError, match="4096"):
        big, _ = uvit(cfg(128, 130, patch=2), 14, "bf16", max_batch=1)      # 65 x 65 = 4225 patches
        big.engine_model(1)
    with pytest.raises(NotImplementedError, match="2\\^32"):                  # the head-major row map: 4089 x 1025^2 >= 2^32
        many, _ = uvit(cfg(128, 128), 15, "bf16", max_batch=4089)
        many.engine_model(4089)
