"""What the sampling-loop tests share (test_guidance, test_autoguidance, test_multistep, test_known_region, test_x0_threshold, test_pag,
test_resample, test_block_cache, test_image_seeds, test_scan_loop, test_scan_exits_loop, test_frag_handoff, test_gpu_parity,
test_long_sequence, test_early_exit, test_early_exit_real): synthetic models on the engine and the configurations they are built from,
seeded inputs, the side stream the loops run on, the development flags as a block, the noise a device loop draws at a step, ONE driver
of the device loops cut into calls (loop_segments, segment_models, run_loop), ONE step-by-step reference of them (run_steps), the
sampler's command line and the error model of the bf16 engine.  tests/test_loop_support_cpu.py tests the planner, the driver's calls and
the draws without a GPU."""
import contextlib

import numpy as np
import torch

from conftest import REPO, TINY
from duodiff_amd.config import ModelParams, load_config
from duodiff_amd.weights import synthetic_state_dict

# bf16 engine vs the reference: the gate on rms(eps - ref) / sigma(ref) is an ERROR MODEL, not a fit to the last run.  Every block rounds
# ~6 GEMM operands to bf16 (norm1 rows, the attention output, norm2 rows, the GELU'd hidden rows, the long-skip copy, P of the attention
# core), each with relative rms 2^-9 / sqrt(3) (uniform rounding error of an 8-bit significand), and the roundings of the `depth` blocks
# add in quadrature on a residual stream of spread ~sigma:  model = 2^-9 / sqrt(3) * sqrt(6 depth)  =  4.8e-3 (depth 3) .. 9.9e-3 (13)
# .. 1.27e-2 (21).  Observed on MI355X (profiles/r05/parity_numbers.txt): 0.47 .. 0.96 of the model.  The bound is the model x 1.5, fixed.
EPS_RMS_MODEL_MARGIN = 1.5

CONFIGS = REPO / "configs"
NULL = 10                                     # the null label of TINY_COND
TINY_COND = dict(TINY, num_classes=11)        # 10 classes + the null row
QA512 = dict(img_size=64, patch_size=4, in_chans=3, embed_dim=512, depth=3, num_heads=8, mlp_ratio=4, qkv_bias=False,
             mlp_time_embed=False, num_classes=-1, normalize_timesteps=True)          # L = 257: attn.qkv inside the attention launch
TAIL256 = dict(img_size=16, patch_size=2, in_chans=3, embed_dim=256, depth=3, num_heads=4, mlp_ratio=4, qkv_bias=False,
               mlp_time_embed=False, num_classes=-1, normalize_timesteps=True)        # the block tail computes the next attn.qkv
KINDS = ["ddpm", "affine", "multistep"]       # the loops every kind of guidance is fused into


def eps_rms_bound(depth):
    return EPS_RMS_MODEL_MARGIN * 2.0 ** -9 / np.sqrt(3.0) * np.sqrt(6.0 * depth)


# ---- models ---------------------------------------------------------------------------------------------------------------------
def uvit(cfg, seed, precision, max_batch=None):
    """a UViT of synthetic weights on the GPU, and its ModelParams"""
    from duodiff_amd.uvit import UViT
    mp = ModelParams.from_dict(cfg)
    m = UViT(**mp.as_dict(), precision=precision, max_batch=max_batch)
    m.load_state_dict(synthetic_state_dict(mp, seed))
    return m.eval().to("cuda"), mp


def ee_uvit(cfg, seed, ctype, precision, max_batch=None):
    """an EarlyExitUViT of synthetic weights (backbone, heads and probes of kind ctype) on the GPU, and its ModelParams"""
    from duodiff_amd.early_exit import EarlyExitUViT
    from duodiff_amd.uvit import UViT
    from duodiff_amd.weights import synthetic_ee_state_dict
    mp = ModelParams.from_dict(cfg)
    m = EarlyExitUViT(UViT(**mp.as_dict(), precision=precision, max_batch=max_batch), ctype)
    m.load_state_dict(synthetic_ee_state_dict(mp, seed, ctype))
    return m.eval().to("cuda"), mp


def tiny_model(max_batch, seed=42, precision="bf16", **cfg):
    """one engine model of dict(TINY, **cfg)"""
    return uvit(dict(TINY, **cfg), seed, precision, max_batch)[0].engine_model(max_batch)


def engine_pair(cfg_a, cfg_b, seeds, max_batch, precision="bf16"):
    """the engine models of two configs (shallow and full, or guide and main) and the second one's ModelParams"""
    m_a, _ = uvit(cfg_a, seeds[0], precision, max_batch)
    m_b, mp = uvit(cfg_b, seeds[1], precision, max_batch)
    return m_a.engine_model(max_batch), m_b.engine_model(max_batch), mp


def celeba_pair(max_batch, seeds=(51, 52)):
    """the product pair at 64 x 64: depth 3 and depth 13, embed_dim 512"""
    return engine_pair(load_config(CONFIGS / "uvit_celeba_3.yaml"), load_config(CONFIGS / "uvit_celeba.yaml"), seeds, max_batch)


def imagenet256_pair(max_batch, seeds):
    """the class-conditional latent pair (4 x 32 x 32, 1000 classes and the null row); the seeds differ between its users"""
    return engine_pair(load_config(CONFIGS / "uvit_imagenet256_3.yaml"), load_config(CONFIGS / "uvit_imagenet256.yaml"), seeds, max_batch)


# ---- inputs: each draw on the CPU generator of its seed (tests/test_loop_support_cpu.py holds the expressions), then moved --------------
def draw_images(B, C, S, seed, scale=1.0):
    x = torch.randn(B, C, S, S, generator=torch.Generator().manual_seed(seed))
    return x if scale == 1.0 else x * scale


def images(B, C, S, seed, scale=1.0):
    return draw_images(B, C, S, seed, scale).cuda()


def draw_labels(B, ncls, seed):
    return torch.randint(0, ncls, (B,), generator=torch.Generator().manual_seed(seed))


def labels(B, ncls, seed):
    return draw_labels(B, ncls, seed).cuda()


def draw_region_inputs(B, seed, C=3, S=8, mask="checker"):
    g = torch.Generator().manual_seed(seed)
    x, x0 = torch.randn(B, C, S, S, generator=g), torch.randn(B, C, S, S, generator=g)
    if mask == "checker":
        i = torch.arange(S)
        m = ((i[:, None] + i[None, :]) % 2).float().expand(B, 1, S, S).clone()
        m[:, :, 1::3, ::2] = 0.5
        m[B - 1] = 1 - m[B - 1]                                   # (the images' masks differ)
    elif mask == "half":
        m = torch.zeros(B, 1, S, S)
        m[..., : S // 2] = 1
    else:
        m = torch.full((B, 1, S, S), float(mask))
    return x, x0, m


def region_inputs(B, seed, C=3, S=8, mask="checker"):
    """x_T, the known image and a mask: a checkerboard with some 0.5 entries, a half image, or a constant"""
    return tuple(v.cuda() for v in draw_region_inputs(B, seed, C, S, mask))


# ---- step tables ------------------------------------------------------------------------------------------------------------------
def ddpm_rows(n, t0=999):
    """the timesteps of n DDPM steps from t0 down: all a `ddpm` loop reads of its rows (z where t > 0)"""
    t = np.arange(t0, t0 - n, -1)
    return dict(t=t.astype(np.float32), noise=(t > 0).astype(np.int32))


def affine_rows(n):
    """n predict_original rows, t = 999 .. 1000 - n: finite a, b and a noise coefficient c > 0 (a DDIM row's c is 0 at eta 0, and at
    eta > 0 the reference's last DDIM row is NaN)"""
    from duodiff_amd import sampler
    ts = list(range(999, 999 - n, -1))
    co = [sampler.affine_coefficients("predict_original", t) for t in ts]
    return dict(t=np.array(ts, np.float32), a=np.array([c[0] for c in co], np.float32), b=np.array([c[1] for c in co], np.float32),
                c=np.array([c[2] for c in co], np.float32), noise=np.array([int(t > 0) for t in ts], np.int32))


def ms_rows(n, kind="sde-dpmsolver++"):
    from duodiff_amd import sampler
    return sampler.multistep_coefficients(kind, sampler.multistep_grid(n), 2)


def first_rows(kind, n):
    """the first n steps from t = 999 of a loop of KINDS"""
    return {"ddpm": ddpm_rows, "affine": affine_rows, "multistep": ms_rows}[kind](n)


# ---- streams and flags ------------------------------------------------------------------------------------------------------------
def side_stream():
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    return s


@contextlib.contextmanager
def dev_flags(ctx, flags):
    """the development flags (dd_dev_set_flags) for the calls inside the block, 0 again behind it whatever happens"""
    ctx.check(ctx.lib.dd_dev_set_flags(ctx.handle, flags))
    try:
        yield
    finally:
        ctx.check(ctx.lib.dd_dev_set_flags(ctx.handle, 0))


# ---- the noise of a step ----------------------------------------------------------------------------------------------------------
def philox_z(em, like, k, seed, stream, y=None, t=500.0):
    """the z a device loop draws at Philox counter k: a one-step dd_sample_affine with the row (0, 0, 1) returns exactly 0 + 0 + 1 * z"""
    from duodiff_amd.engine import sample_affine_loop
    z = like.clone()
    with torch.cuda.stream(stream):
        sample_affine_loop(em.ctx, em, None, z, [t], [0.0], [0.0], [1.0], [1], y=y, seed=seed, counter_base=k, noise="philox",
                           use_graph=False, stream=stream)
    stream.synchronize()
    return z


def philox_z2(em, like, k, seed, stream, y=None):
    """the z2 of a step: a one-step region call with m = 1, x0 = 0, ka = 0, kb = 1 on the row (0, 0, 0) returns 1 * (0 + 1 * z2) + 0 * 0"""
    from duodiff_amd.engine import KnownRegion, sample_affine_region_loop
    z = like.clone()
    B, _, S, _ = like.shape
    reg = KnownRegion(torch.zeros_like(like), torch.ones(B, 1, S, S, device="cuda"), np.zeros(1, np.float32), np.ones(1, np.float32))
    with torch.cuda.stream(stream):
        sample_affine_region_loop(em.ctx, em, None, z, reg, [500.0], [0.0], [0.0], [0.0], [0], y=y, seed=seed, counter_base=k,
                                  noise="philox", use_graph=False, stream=stream)
    stream.synchronize()
    return z


def philox_z3(em, like, k, seed, stream, y=None):
    """the z3 a jump draws at Philox counter k: a one-row walk call on x = 0 with the jump row (ja, jc) = (0, 1) returns 0 * 0 + 1 * z3"""
    from duodiff_amd.engine import sample_affine_walk_loop
    z = torch.zeros_like(like)
    rows = dict(t=[500.0], a=[0.0], b=[0.0], c=[1.0], noise=[1], jump=[1])
    with torch.cuda.stream(stream):
        sample_affine_walk_loop(em.ctx, em, None, z, rows, y=y, seed=seed, counter_base=k, noise="philox", use_graph=False, stream=stream)
    stream.synchronize()
    return z


def known_region(plan, x0, mask, k0=0, k1=None):
    from duodiff_amd import sampler
    from duodiff_amd.engine import KnownRegion
    ka, kb = sampler.known_rows(plan)
    return KnownRegion(x0, mask, ka[k0:k1], kb[k0:k1])


def _rows_and_region(rows_or_plan, region):
    """(the row arrays, the region as a KnownRegion of one (ka, kb) per row or None); region: a KnownRegion, or (x0, mask) beside a plan"""
    rows = getattr(rows_or_plan, "rows", rows_or_plan)
    if region is not None and not hasattr(region, "ka"):
        region = known_region(rows_or_plan, *region)
    return rows, region


# ---- the device loop, cut into calls ------------------------------------------------------------------------------------------------
def loop_segments(n, cuts=(), switch_after=None):
    """A loop of n rows as the calls [0, *cuts, n] -- cuts holds the ROW AT WHICH A NEW CALL STARTS (a loop "cut after step c" passes
    c + 1) -- as (k0, k1, sw): sw is the call's own switch_after, counted from k0 and clamped to the call (None: the loop has no switch)"""
    bounds = [0, *cuts, n]
    for k0, k1 in zip(bounds[:-1], bounds[1:]):
        yield k0, k1, None if switch_after is None else min(max(switch_after - k0, 0), k1 - k0)


def segment_models(first, late, sw, n):
    """(the model that starts a call of n rows, the one it switches to inside it or None): the late model starts the call when sw == 0
    and is passed as the call's late model only when 0 < sw < n"""
    return late if sw == 0 else first, late if sw and sw < n else None


def run_loop(kind, first, x_in, rows_or_plan, stream, *, h0=None, **kw):
    """The device loop `kind` -- ddpm, affine, multistep (threshold: the same), walk, cached -- on a copy of x_in (h: zero, or a copy of
    h0), cut into the calls of loop_segments with h and the Philox counter carried over -> (x, h, chains of the last call).  See loop_calls."""
    x, h = x_in.clone(), torch.zeros_like(x_in) if h0 is None else h0.clone()
    with torch.cuda.stream(stream):
        return x, h, loop_calls(kind, first, x, h, rows_or_plan, stream, **kw)


def loop_calls(kind, first, x, h, rows_or_plan, stream, *, late=None, switch_after=None, region=None, threshold=None, cache=None, cuts=(),
               flags=0, seed=5, noise="philox", use_graph=True, guidance=None, y=None, image_seeds=None, **entry_kw):
    """run_loop on the stream that is current, in place on x and h -> chains.  rows_or_plan: a StepPlan or its rows; region: a
    KnownRegion of one (ka, kb) per row of the loop, or (x0, mask) beside a plan; threshold: an X0Threshold (the thresholded multistep
    entry); cache: (blocks, order) of a cached loop; entry_kw: what only one entry takes (dd_sample's t_switch).  Every call gets its
    slice of every row array and of the region's rows and counter_base = its first row -- `ddpm` t_start / t_end from its t instead,
    and the models whole: that loop switches by timestep.  `walk` gets the models whole too and switch_after - k0 unclamped: its rows
    name their model.  The other kinds get segment_models'.  The whole run goes under the development flags `flags` and image_seeds."""
    from duodiff_amd import engine
    ctx = first.ctx
    rows, region = _rows_and_region(rows_or_plan, region)
    if late is None:
        switch_after = None
    with dev_flags(ctx, flags), ctx.image_seeds(image_seeds, stream):
        for k0, k1, sw in loop_segments(len(rows["t"]), cuts, switch_after):
            seg = {k: v[k0:k1] for k, v in rows.items()}
            reg = None if region is None else region._replace(ka=region.ka[k0:k1], kb=region.kb[k0:k1])
            known = () if reg is None else (reg,)
            m0, m1 = segment_models(first, late, sw, k1 - k0)
            kw = dict(y=y, seed=seed, noise=noise, use_graph=use_graph, stream=stream, guidance=guidance, **entry_kw)
            if kind == "ddpm":
                (engine.sample_region_loop if known else engine.sample_loop)(
                    ctx, first, late, x, *known, t_start=int(seg["t"][0]), t_end=int(seg["t"][-1]), **kw)
                continue
            kw.update(counter_base=k0, switch_after=sw)
            if kind == "affine":
                (engine.sample_affine_region_loop if known else engine.sample_affine_loop)(
                    ctx, m0, m1, x, *known, seg["t"], seg["a"], seg["b"], seg["c"], seg["noise"], **kw)
            elif kind in ("multistep", "threshold") and threshold is not None:
                engine.sample_multistep_threshold_loop(ctx, m0, m1, x, h, seg, threshold, region=reg, **kw)
            elif kind in ("multistep", "threshold"):
                (engine.sample_multistep_region_loop if known else engine.sample_multistep_loop)(ctx, m0, m1, x, *known, h, seg, **kw)
            elif kind == "walk":
                kw.update(switch_after=None if switch_after is None else switch_after - k0)
                engine.sample_affine_walk_loop(ctx, first, late, x, seg, region=reg, **kw)
            elif kind == "cached":
                engine.sample_affine_cached_loop(ctx, m0, m1, x, seg, blocks=cache[0], order=cache[1], region=reg, **kw)
            else:
                raise ValueError(f"no device loop of kind {kind!r}")
        stream.synchronize()
        return ctx.lib.dd_dev_last_sample_chains(ctx.handle)


def run_first_steps(kind, first, late, x0, stream, *, switch, n=8, seed=0, **kw):
    """The first n steps from t = 999 of a loop of KINDS on a copy of x0: DDPM (late after `switch` steps), n predict_original rows or
    DPM-Solver++-n (late from step `switch`); kw: run_loop's -> x (multistep: x and h stacked)"""
    sw = dict(t_switch=switch) if kind == "ddpm" else dict(switch_after=switch)
    x, h, _ = run_loop(kind, first, x0, first_rows(kind, n), stream, late=late, seed=seed, **sw, **kw)
    return x if kind != "multistep" else torch.stack([x, h])


# ---- the same loop, one step at a time ------------------------------------------------------------------------------------------------
def run_steps(kind, first, x_in, rows_or_plan, stream, *, late=None, switch_after=None, region=None, threshold=None, cache=None, seed=5,
              noise="philox", guidance=None, y=None, image_seeds=None, with_z2=True, sticky_late=False):
    """The reference of run_loop, from the unfused public entry points alone: per row forward[_guided | _autoguided | _perturbed |
    _cached] of the row's model, then ddpm_step / affine_step / multistep_step / threshold_step (a walk's jump row: jump_step and no
    model), then known_blend where a region is given -- fed the z, z2 and z3 the device loop draws at the row's counter (the timestep in
    `ddpm`, else the row index; noise "none": none of them; with_z2 False: no z2) -> (x, h).  The late model runs from row
    switch_after on; in a walk where late[k] is set (sticky_late: and from then on, what one switch_after could express).  A model
    takes y iff it is class-conditional."""
    from duodiff_amd.engine import Autoguidance, Perturbed
    ctx = first.ctx
    rows, region = _rows_and_region(rows_or_plan, region)
    x, h, eps = x_in.clone(), torch.zeros_like(x_in), torch.empty_like(x_in)
    draws, switched = noise == "philox", False
    with ctx.image_seeds(image_seeds, stream):
        for k in range(len(rows["t"])):
            t = float(rows["t"][k])
            ctr = int(t) if kind == "ddpm" else k
            if kind == "walk" and rows["jump"][k]:
                z3 = philox_z3(first, x_in, ctr, seed, stream, y if first.mp.num_classes > 0 else None) if draws else None
                with torch.cuda.stream(stream):
                    ctx.jump_step(x, z3, rows["a"][k], rows["c"][k], out=x, stream=stream)
                continue
            if kind == "walk":
                switched = switched or bool(rows["late"][k])
                m = late if rows["late"][k] or (sticky_late and switched) else first
            else:
                m = late if switch_after is not None and k >= switch_after else first
            ym = y if m.mp.num_classes > 0 else None
            z = philox_z(m, x_in, ctr, seed, stream, ym) if draws and rows["noise"][k] else None
            z2 = philox_z2(m, x_in, ctr, seed, stream, ym) if draws and with_z2 and region is not None and region.kb[k] != 0 else None
            with torch.cuda.stream(stream):
                if cache is not None:
                    m.forward_cached(x, t, ym, blocks=cache[0], op=int(rows["cache"][k]), w=float(rows["cw"][k]), guidance=guidance, out=eps,
                                     stream=stream)
                elif isinstance(guidance, Autoguidance):
                    if m is guidance.guide:
                        m.forward(x, t, ym, out=eps, stream=stream)
                    else:
                        m.forward_autoguided(x, t, y, guidance.guide, guidance.scale, out=eps, stream=stream)
                elif isinstance(guidance, Perturbed):
                    m.forward_perturbed(x, t, ym, guidance.scale, guidance.layers_first if m is first else guidance.layers_late, out=eps,
                                        stream=stream)
                elif guidance is not None:
                    m.forward_guided(x, t, ym, guidance[0], guidance[1], out=eps, stream=stream)
                else:
                    m.forward(x, t, ym, out=eps, stream=stream)
                if kind == "ddpm":
                    ctx.ddpm_step(x, eps, z, int(t), out=x, stream=stream)
                elif threshold is not None:
                    ctx.threshold_step(x, eps, z, h, threshold, *(rows[c][k] for c in "abcdpq"), rows["hist"][k], out=x, stream=stream)
                elif kind in ("multistep", "threshold"):
                    ctx.multistep_step(x, eps, z, h, *(rows[c][k] for c in "abcdpq"), rows["hist"][k], out=x, stream=stream)
                else:
                    ctx.affine_step(x, eps, z, rows["a"][k], rows["b"][k], rows["c"][k], out=x, stream=stream)
                if region is not None:
                    ctx.known_blend(x, region.x0, region.mask, z2, region.ka[k], region.kb[k], out=x, stream=stream)
    stream.synchronize()
    return x, h


def cli_argv(config, *extra, par="predict_noise"):
    return ["--checkpoint_path", "/nonexistent.pth", "--batch_size", "2", "--parametrization", par,
            "--output_folder", "/tmp/unused", "--config_path", str(config), *extra]
