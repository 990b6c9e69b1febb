"""Block caching (DeepCache, Ma et al. 2024; order 1: TaylorSeer) on the GPU: cache_extrapolate_kernel<T> (csrc/cache.hip), dd_forward_cached,
dd_sample_affine_cached, get_samples(cache=...) and the sampler options --cache_blocks / --cache_interval / --cache_order.

Kernel: per element against float64 of the same stored operands, |out - ref| <= half an ulp of ref in the activation type (bf16 mode)
+ 2^-22 (|last| + |w| (|last| + |prev|)) (tests/test_block_cache_cpu.py extrapolate_ref), canary rows intact.
Forward: against the unchanged numpy oracle, the reuse pass composed by patching oracle.uvit_oracle.block_forward to return y^ for the deep
blocks; y^ comes from the taps of earlier oracle runs.  fp32 max <= 1e-4, for every op; bf16 rms <= eps_rms_bound(depth) sigma for a refresh
and an order-0 reuse, x (1 + 2 |w|) for order 1 in bf16 alone (the cached rows' roundings are amplified by at most that) -- the project's
own bounds; under guidance both x (1 + 2 s).  Before
the engine is asked, the oracle's reuse output must differ from its own full output by >= 3 x the bf16 bound, and order 1 from order 0 by
>= 2 x order 1's bound: a test of nothing fails itself.
Loops: against their own building blocks, bit for bit."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest
import torch

import kernel_support
from conftest import REPO, TINY
from duodiff_amd import _lib as L
from duodiff_amd import step_plan as sp
from duodiff_amd.config import ModelParams
from duodiff_amd.weights import synthetic_state_dict
from kernel_support import NAN16, NAN32, P, bf16_bits, from_bf16_bits, gate
from loop_support import QA512, TAIL256, TINY_COND, dev_flags, engine_pair, eps_rms_bound, images, known_region, labels, run_loop, run_steps
from loop_support import side_stream, uvit
from test_block_cache_cpu import extrapolate_operands, extrapolate_ref

gpu = pytest.mark.gpu


# ---- GPU, the kernel ---------------------------------------------------------------------------------------------------------
# (B, L, D); the last one is more than one pass of the capped grid: 2048 workgroups x 256 lanes x 8 bf16 = 4 194 304 elements
KERNEL_SIZES = [(1, 17, 64), (3, 258, 512), (2, 257, 1024), (17, 258, 1024)]


def _run_kernel(prec, last, prev, op, w, table=1):
    ctx = kernel_support.ctx()
    rows, D = last.shape
    bf = prec == "bf16"
    out = np.full((rows + 8, D), 0xA5A5 if bf else 0xA5A5A5A5, np.uint16 if bf else np.uint32)
    ops = [bf16_bits(v) if bf else np.ascontiguousarray(v, np.float32) for v in (last, prev)]
    st = ctx.lib.dd_dev_cache_extrapolate(ctx.handle, 0 if bf else 1, rows, D, P(ops[0]), P(ops[1]), op, w, table, P(out), 0, None,
                                          C.byref(C.c_float(0)))
    assert st == L.DD_OK, ctx.lib.dd_last_error(ctx.handle).decode()
    assert (out[rows:] == (NAN16 if bf else NAN32)).all(), "canary rows behind the output were written"
    return out[:rows], (from_bf16_bits(out[:rows]) if bf else out[:rows].view(np.float32))


@gpu
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("sigma", [1.0, 100.0])
@pytest.mark.parametrize("w", [0.5, 1.0, -0.25, 2.0])
@pytest.mark.parametrize("size", KERNEL_SIZES)
def test_cache_extrapolate_against_float64_reference(size, w, sigma, prec):
    """out aliases neither input (include/duodiff_dev.h): three buffers.  The op and w travel through the device table row, as in a loop."""
    B, L_, D = size
    last, prev = extrapolate_operands(B * L_, D, sigma, prec, 1000 + D + B)
    ref, tol = extrapolate_ref(last, prev, w, prec)
    _, got = _run_kernel(prec, last, prev, 2, w)
    r = gate(got, ref, tol, f"cache_extrapolate {size} w={w} sigma={sigma} {prec}")
    print(f"cache_extrapolate {size} w={w} sigma={sigma} {prec}: max err/bound {r:.3f}")


@gpu
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_cache_extrapolate_ops_and_argument_form(prec):
    """op 1 (and 0) copy last bit for bit and never read prev (NaN there stays out); the launch's argument form (no table) gives the
    table form's bits"""
    last, prev = extrapolate_operands(3 * 17, 128, 1.0, prec, 5)
    nan = np.full_like(prev, np.nan)
    want = bf16_bits(last) if prec == "bf16" else last.view(np.uint32)
    for op in (0, 1):
        for table in (0, 1):
            bits, vals = _run_kernel(prec, last, nan, op, 1.0, table)
            assert np.isfinite(vals).all() and np.array_equal(bits, want), f"op {op} table {table}"
    a, _ = _run_kernel(prec, last, prev, 2, 0.5, 1)
    b, _ = _run_kernel(prec, last, prev, 2, 0.5, 0)
    assert np.array_equal(a, b) and not np.array_equal(a, want)


@gpu
def test_cache_extrapolate_rejects_bad_arguments():
    ctx = kernel_support.ctx()
    last = np.zeros((4, 64), np.float32)
    out = np.full((12, 64), 0xA5A5A5A5, np.uint32)
    for rows, D, op in ((0, 64, 2), (4, 32, 2), (4, 96, 2), (4, 64, 3), (4, 64, -1)):
        st = ctx.lib.dd_dev_cache_extrapolate(ctx.handle, 1, rows, D, P(last), P(last), op, 1.0, 1, P(out), 0, None, C.byref(C.c_float(0)))
        assert st == L.DD_ERR_INVALID and (out == 0xA5A5A5A5).all()


# ---- GPU, the forward against the oracle -----------------------------------------------------------------------------------------
IMNET64_768 = dict(img_size=64, patch_size=4, in_chans=3, embed_dim=768, depth=5, num_heads=12, mlp_ratio=4, qkv_bias=False,
                   mlp_time_embed=False, num_classes=11, normalize_timesteps=False)          # row-resident launches, class-conditional
IMNET256_1024 = dict(img_size=32, patch_size=2, in_chans=4, embed_dim=1024, depth=5, num_heads=16, mlp_ratio=4, qkv_bias=False,
                     mlp_time_embed=False, num_classes=11, normalize_timesteps=False)        # split-K
# name: (config, depth, K, B, dev flags)
FORWARD_CASES = {}
for _name, _cfg, _B, _flags_ in (("tiny", TINY, 3, 0), ("tail256", TAIL256, 3, 0), ("qa512", QA512, 2, 0),
                                 ("qa512_no_fused_qa", QA512, 2, L.DD_DEV_NO_FUSED_QA), ("imnet64_768", IMNET64_768, 2, 0),
                                 ("imnet256_1024", IMNET256_1024, 2, 0)):
    for _K in (1, 2):
        FORWARD_CASES[f"{_name}_d5_k{_K}"] = (_cfg, 5, _K, _B, _flags_)
FORWARD_CASES["tiny_d3_k1"] = (TINY, 3, 1, 3, 0)                 # only the mid block is skipped
FORWARD_CASES["tiny_d7_k3"] = (TINY, 7, 3, 3, 0)                 # K = h: again only the mid block, behind three in-blocks
TS = (900.0, 850.0, 800.0)
W = 1.0
# Where three unit-variance inputs leave the oracle's own distances short of the factors below, the inputs are spread: at depth 7 with
# K = 3 only the mid block is skipped behind three in-blocks and y^ passes three more out-blocks of small synthetic weights (reuse moves
# eps by 0.015 sigma, order 1 by 0.015 sigma); with the second input at 16 sigma they are 0.127 and 0.086 against 0.033 and 0.066.
STORY = {"tiny_d7_k3": dict(x_scale=(1.0, 16.0, 1.0))}


def _block_names(depth):
    half = depth // 2
    return [f"in_blocks.{i}" for i in range(half)] + ["mid_block"] + [f"out_blocks.{i}" for i in range(half)]


def _oracle(cfg, seed):
    import oracle
    mp = ModelParams.from_dict(cfg)
    sd = synthetic_state_dict(mp, seed)
    return oracle.UViTOracle(mp.as_dict(), {k: v.numpy() for k, v in sd.items()}), mp


def _oracle_reuse(monkeypatch, orc, depth, K, x, t, y, y_hat):
    """the oracle's reuse pass: oracle.uvit_oracle.block_forward returns y^ for the deep blocks K .. depth - 1 - K, so out-block
    depth - K takes y^ for its x operand and block K - 1's output for its long skip"""
    from oracle import uvit_oracle as uo
    deep = {n + "." for n in _block_names(depth)[K:depth - K]}
    real = uo.block_forward

    def block_forward(xx, p, prefix, num_heads, skip=None):
        return y_hat if prefix in deep else real(xx, p, prefix, num_heads, skip=skip)

    with monkeypatch.context() as mpatch:
        mpatch.setattr(uo, "block_forward", block_forward)
        return orc(x, np.full((x.shape[0],), t, np.float32), y).astype(np.float64)


def _oracle_story(monkeypatch, cfg, depth, K, B, y=None, seeds=(61, 62), ts=None, x_scale=(1.0, 1.0, 1.0)):
    """Three independent inputs at TS; the oracle's full outputs, the deep outputs y_deep of the first two, its order-0 and order-1 reuse
    outputs at the third, and its reuse output at the second input itself (which is its full output there)"""
    cfg = dict(cfg, depth=depth)
    orc, mp = _oracle(cfg, seeds[0])
    g = torch.Generator().manual_seed(seeds[1])
    ts = TS if ts is None else ts
    xs = [sc * torch.randn(B, mp.in_chans, mp.img_size, mp.img_size, generator=g) for sc in x_scale]
    deep_name = _block_names(depth)[depth - 1 - K]
    full, deep = [], []
    for x, t in zip(xs, ts):
        taps = {}
        full.append(orc(x.numpy(), np.full((B,), t, np.float32), y, taps=taps).astype(np.float64))
        deep.append(taps[deep_name])
    y0 = deep[1]
    y1 = (deep[1].astype(np.float64) + W * (deep[1].astype(np.float64) - deep[0].astype(np.float64))).astype(np.float32)
    reuse0 = _oracle_reuse(monkeypatch, orc, depth, K, xs[2].numpy(), ts[2], y, y0)
    reuse1 = _oracle_reuse(monkeypatch, orc, depth, K, xs[2].numpy(), ts[2], y, y1)
    same = _oracle_reuse(monkeypatch, orc, depth, K, xs[1].numpy(), ts[1], y, y0)
    return cfg, mp, xs, full, reuse0, reuse1, same


def _rms(a):
    return float(np.sqrt((np.asarray(a, np.float64) ** 2).mean()))


def _not_vacuous(depth, full3, reuse0, reuse1, what):
    sigma = float(full3.std())
    bound = eps_rms_bound(depth)
    d_reuse, d_order = _rms(reuse0 - full3) / sigma, _rms(reuse1 - reuse0) / sigma
    print(f"{what}: the oracle's reuse moves eps by {d_reuse:.4f} sigma, order 1 against order 0 by {d_order:.4f} sigma (bf16 bound {bound:.4f})")
    assert d_reuse >= 3 * bound, f"{what}: the oracle's reuse output is too close to its full output to test anything"
    assert d_order >= 2 * bound * (1 + 2 * abs(W)), f"{what}: the oracle's order 1 is too close to its order 0 to test anything"
    return sigma


def _check(got, want, prec, depth, sigma, what, factor=1.0, amp=1.0):
    """fp32: max <= 1e-4 x factor; bf16: rms <= eps_rms_bound(depth) x factor x amp sigma.  factor: the guided combination's 1 + 2 s, on both
    types; amp: order 1's 1 + 2 |w| on the cached rows' bf16 roundings, on the bf16 bound alone"""
    got = got.cpu().numpy().astype(np.float64) if torch.is_tensor(got) else np.asarray(got, np.float64)
    assert np.isfinite(got).all(), what
    sigma = float(want.std())                                     # (of this reference: the inputs of a story may differ in scale)
    err, rms = float(np.abs(got - want).max()), _rms(got - want)
    bound = 1e-4 * factor if prec == "fp32" else eps_rms_bound(depth) * factor * amp
    print(f"{what} {prec}: max {err:.3e} rms {rms / sigma:.5f} sigma (bound: {'max' if prec == 'fp32' else 'rms / sigma'} <= {bound:.3e})")
    if prec == "fp32":
        assert err <= bound, what
    else:
        assert rms <= bound * sigma, what


@gpu
@pytest.mark.parametrize("case", sorted(FORWARD_CASES))
def test_forward_cached_vs_oracle(monkeypatch, case):
    cfg, depth, K, B, flags = FORWARD_CASES[case]
    gy = torch.Generator().manual_seed(63)
    y = torch.randint(0, 11, (B,), generator=gy) if cfg["num_classes"] > 0 else None
    yn = None if y is None else y.numpy()
    cfg, mp, xs, full, reuse0, reuse1, same = _oracle_story(monkeypatch, cfg, depth, K, B, yn, **STORY.get(case, {}))
    sigma = _not_vacuous(depth, full[2], reuse0, reuse1, case)
    assert _rms(same - full[1]) <= 1e-5 * sigma                   # (the composition itself: y^ at its own input is the full pass)
    yd = None if y is None else y.cuda()
    xd = [x.cuda() for x in xs]
    for prec in ("fp32", "bf16"):
        with dev_flags(kernel_support.ctx(), flags):
            m, _ = uvit(cfg, 61, prec, max_batch=B)
            em = m.engine_model(B)
        r1 = em.forward_cached(xd[0], TS[0], yd, blocks=K, op=0)
        r2 = em.forward_cached(xd[1], TS[1], yd, blocks=K, op=0)
        plain2 = em.forward(xd[1], TS[1], yd)
        again = em.forward_cached(xd[1], TS[1], yd, blocks=K, op=1)
        u0 = em.forward_cached(xd[2], TS[2], yd, blocks=K, op=1)
        u1 = em.forward_cached(xd[2], TS[2], yd, blocks=K, op=2, w=W)
        u0_again = em.forward_cached(xd[2], TS[2], yd, blocks=K, op=1)
        torch.cuda.synchronize()
        _check(r1, full[0], prec, depth, sigma, f"{case}: refresh 1")
        _check(r2, full[1], prec, depth, sigma, f"{case}: refresh 2")
        _check(plain2, full[1], prec, depth, sigma, f"{case}: dd_forward")
        _check(again, full[1], prec, depth, sigma, f"{case}: reuse at the refresh's own input")
        _check(u0, reuse0, prec, depth, sigma, f"{case}: order-0 reuse")
        _check(u1, reuse1, prec, depth, sigma, f"{case}: order-1 reuse", amp=1 + 2 * abs(W))
        # a refresh's eps is dd_forward's: to the same bounds directly, and on the GEMM path, where caching changes no launch of a
        # refresh but the copy of y_deep, bit for bit in fp32
        _check(r2, plain2.cpu().numpy().astype(np.float64), prec, depth, sigma, f"{case}: refresh 2 against dd_forward")
        if prec == "fp32" and case.startswith("tiny"):
            assert torch.equal(r2, plain2), "a GEMM-path refresh in fp32 is not dd_forward's eps bit for bit"
        assert torch.equal(u0, u0_again), "a reuse step changed the cache"
        if prec == "fp32":       # the engine tells the orders apart as the oracle does
            assert _rms(u1.cpu().numpy() - u0.cpu().numpy()) >= 0.5 * _rms(reuse1 - reuse0)
        del em, m


@gpu
def test_forward_cached_guided_vs_oracle(monkeypatch):
    """Classifier-free guidance: the cache holds the 2 B rows; eps = eps_c + s (eps_c - eps_u) of two oracle compositions, conditional and
    null-labelled, each with the y^ of its own earlier runs; bound x (1 + 2 s)"""
    depth, K, B, s, null = 5, 1, 3, 0.7, 10
    y = torch.randint(0, 10, (B,), generator=torch.Generator().manual_seed(63))
    sides = [_oracle_story(monkeypatch, TINY_COND, depth, K, B, lab) for lab in (y.numpy(), np.full((B,), null, np.int64))]
    cfg, mp, xs = sides[0][:3]

    def guided(i):
        c, u = sides[0][i], sides[1][i]
        return [cc + s * (cc - uu) for cc, uu in zip(c, u)] if isinstance(c, list) else c + s * (c - u)

    full, reuse0, reuse1 = guided(3), guided(4), guided(5)
    sigma = _not_vacuous(depth, full[2], reuse0, reuse1, "guided")
    xd, yd = [x.cuda() for x in xs], y.cuda()
    for prec in ("fp32", "bf16"):
        m, _ = uvit(cfg, 61, prec, max_batch=2 * B)
        em = m.engine_model(2 * B)
        kw = dict(blocks=K, guidance=(s, null))
        r1 = em.forward_cached(xd[0], TS[0], yd, op=0, **kw)
        r2 = em.forward_cached(xd[1], TS[1], yd, op=0, **kw)
        g2 = em.forward_guided(xd[1], TS[1], yd, s, null)
        u0 = em.forward_cached(xd[2], TS[2], yd, op=1, **kw)
        u1 = em.forward_cached(xd[2], TS[2], yd, op=2, w=W, **kw)
        torch.cuda.synchronize()
        f = 1 + 2 * s
        _check(r1, full[0], prec, depth, sigma, "guided: refresh 1", factor=f)
        _check(r2, full[1], prec, depth, sigma, "guided: refresh 2", factor=f)
        _check(g2, full[1], prec, depth, sigma, "guided: dd_forward_guided", factor=f)
        _check(u0, reuse0, prec, depth, sigma, "guided: order-0 reuse", factor=f)
        _check(u1, reuse1, prec, depth, sigma, "guided: order-1 reuse", factor=f, amp=1 + 2 * abs(W))
        _check(r2, g2.cpu().numpy().astype(np.float64), prec, depth, sigma, "guided: refresh 2 against dd_forward_guided", factor=f)
        # an unguided call of B rows finds no refresh of its geometry
        with pytest.raises(ValueError, match="no refresh"):
            em.forward_cached(xd[2], TS[2], yd, blocks=K, op=1)
        del em, m


# ---- GPU, the loops --------------------------------------------------------------------------------------------------------------
def _pair(max_batch, cond=False, seeds=(41, 42)):
    base = TINY_COND if cond else TINY
    return engine_pair(dict(base, depth=3), dict(base, depth=5), seeds, max_batch)[:2]


def _plan(kind, n, N, order, late=True, t_switch=4, K=1, **kw):
    """DDIM rows, or the predict_noise DDPM rows (c > 0: the Philox draw shows); with `late` the switch falls on step 4, a reuse position
    of the first model under N = 3"""
    if kind == "ddim":
        return sp.step_plan("predict_noise", use_ddim=True, ddim_steps=n + 1, has_late=late, t_switch=1000 - 600 if late else np.inf,
                            cache_blocks=K, cache_interval=N, cache_order=order, **kw)
    return sp.step_plan("predict_noise", num_steps=n, has_late=late, t_switch=t_switch if late else np.inf, cache_blocks=K,
                        cache_interval=N, cache_order=order, **kw)


def _device(plan, K, order, first, late, x0, stream, *, cuts=(), seed=0, **kw):
    """the plan as device loop calls on a copy of x0, cut AFTER the steps `cuts`; kw: run_loop's (region: a KnownRegion) -> x"""
    return run_loop("cached", first, x0, plan, stream, late=late, switch_after=plan.switch_after, cache=(K, order), cuts=[c + 1 for c in cuts],
                    seed=seed, **kw)[0]


def _manual(plan, K, first, late, x0, stream, *, seed=0, noise="none", **kw):
    """forward_cached + affine_step [+ known_blend] per step, z and z2 as the device loop draws them"""
    return run_steps("cached", first, x0, plan, stream, late=late, switch_after=plan.switch_after, cache=(K, None), seed=seed, noise=noise, **kw)[0]


@gpu
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("kind,noise", [("ddim", "none"), ("ddpm", "none"), ("ddpm", "philox")])
def test_cached_loop_equals_manual_steps(kind, noise, order):
    """9 steps on the pair (depths 3 and 5, K = 1), N = 3, the switch on a reuse position of the first model: the device loop, graph-replayed
    and eager, == forward_cached + affine_step per step; and the cache moves the result"""
    from duodiff_amd.engine import sample_affine_loop
    B = 4
    es, ef = _pair(B)
    x0, stream = images(B, 3, 8, 11), side_stream()
    plan = _plan(kind, 9, 3, order)
    assert plan.switch_after is not None and plan.rows["cache"][plan.switch_after] == 0 and (plan.switch_after % 3) != 0
    assert (2 in plan.rows["cache"]) == (order == 1)
    kw = dict(seed=21, noise=noise)
    loops = [_device(plan, 1, order, es, ef, x0, stream, use_graph=ug, **kw) for ug in (True, False)]
    manual = _manual(plan, 1, es, ef, x0, stream, **kw)
    r = plan.rows
    plain = x0.clone()
    with torch.cuda.stream(stream):
        sample_affine_loop(es.ctx, es, ef, plain, r["t"], r["a"], r["b"], r["c"], r["noise"], switch_after=plan.switch_after, stream=stream, **kw)
        stream.synchronize()
    assert torch.isfinite(manual).all() and not torch.equal(manual, x0)
    assert torch.equal(loops[0], loops[1]), "graph replay differs from eager launches"
    assert torch.equal(loops[0], manual), "the cached loop differs from its manual steps"
    assert not torch.equal(loops[0], plain), "the cached loop equals the uncached loop: nothing was reused"


@gpu
def test_interval_one_equals_the_uncached_affine_loop():
    """N = 1: every step refreshes -- the full forward with the seam's skip_linear unfused; fp32 mode runs the same GEMMs either way"""
    from duodiff_amd.engine import sample_affine_loop
    B = 4
    es, ef, _ = engine_pair(dict(TINY, depth=3), dict(TINY, depth=5), (41, 42), B, precision="fp32")
    x0, stream = images(B, 3, 8, 12), side_stream()
    plan = _plan("ddpm", 6, 1, 0)
    got = _device(plan, 1, 0, es, ef, x0, stream, seed=3, noise="philox")
    r, plain = plan.rows, x0.clone()
    with torch.cuda.stream(stream):
        sample_affine_loop(es.ctx, es, ef, plain, r["t"], r["a"], r["b"], r["c"], r["noise"], switch_after=plan.switch_after, seed=3,
                           noise="philox", stream=stream)
        stream.synchronize()
    assert torch.equal(got, plain)


@gpu
@pytest.mark.parametrize("order", [0, 1])
def test_cached_two_chains_equal_one_chain(order):
    B = 6
    es, ef = _pair(B)
    x0, stream = images(B, 3, 8, 13), side_stream()
    plan = _plan("ddpm", 9, 3, order)
    outs = {}
    for name, flags in (("chained", L.DD_DEV_FORCE_CHAINS), ("single", L.DD_DEV_NO_CHAINS)):
        outs[name] = (_device(plan, 1, order, es, ef, x0, stream, seed=23, noise="philox", flags=flags), es.ctx.lib.dd_dev_last_sample_chains(es.ctx.handle))
    assert outs["chained"][1] == 2 and outs["single"][1] == 1
    assert torch.isfinite(outs["single"][0]).all()
    assert torch.equal(outs["chained"][0], outs["single"][0]), "cached chains differ from the single chain"


@gpu
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("flags", [0, L.DD_DEV_FORCE_CHAINS])
def test_a_cut_cached_loop_equals_the_uncut_one(flags, order):
    """cut after steps 2 and 5, both reuse rows (N = 3; under order 1 step 5 extrapolates), and after steps 1 and 4: the caches carry over the calls"""
    B = 4
    es, ef = _pair(B)
    x0, stream = images(B, 3, 8, 14), side_stream()
    plan = _plan("ddpm", 9, 3, order, t_switch=7)
    assert list(plan.rows["cache"][:7]) == [0, 1, 1, 0, 2 if order else 1, 2 if order else 1, 0]
    whole = _device(plan, 1, order, es, ef, x0, stream, seed=25, noise="philox", flags=flags)
    for cuts in ((2, 5), (1, 4)):      # behind reuse rows; and in front of them: rows 2 and 5 then open a call on an earlier call's cache
        cut = _device(plan, 1, order, es, ef, x0, stream, cuts=cuts, seed=25, noise="philox", flags=flags)
        assert torch.equal(cut, whole), f"cut after steps {cuts} differs from the uncut loop"
    assert torch.isfinite(whole).all()


@gpu
def test_cached_loop_with_a_known_region_equals_manual_steps():
    B = 4
    es, ef = _pair(B)
    x0, stream = images(B, 3, 8, 15), side_stream()
    plan = _plan("ddpm", 9, 3, 1)
    g = torch.Generator().manual_seed(16)
    region = known_region(plan, torch.randn(B, 3, 8, 8, generator=g).cuda(), (torch.rand(B, 1, 8, 8, generator=g) > 0.5).float().cuda())
    got = _device(plan, 1, 1, es, ef, x0, stream, region=region, seed=27, noise="philox")
    manual = _manual(plan, 1, es, ef, x0, stream, region=region, seed=27, noise="philox")
    free = _device(plan, 1, 1, es, ef, x0, stream, seed=27, noise="philox")
    assert torch.isfinite(got).all() and torch.equal(got, manual) and not torch.equal(got, free)


@gpu
@pytest.mark.parametrize("flags", [0, L.DD_DEV_FORCE_CHAINS])
def test_cached_loop_with_cfg_equals_manual_guided_steps(flags):
    B, g = 4, (0.7, 10)
    es, ef = _pair(2 * B, cond=True)
    x0, stream = images(B, 3, 8, 17), side_stream()
    y = labels(B, 10, 18)
    plan = _plan("ddpm", 9, 3, 1)
    got = _device(plan, 1, 1, es, ef, x0, stream, seed=29, noise="philox", guidance=g, y=y, flags=flags)
    manual = _manual(plan, 1, es, ef, x0, stream, seed=29, noise="philox", guidance=g, y=y)
    unguided = _device(plan, 1, 1, es, ef, x0, stream, seed=29, noise="philox", guidance=(0.0, 10), y=y)
    assert torch.isfinite(got).all() and torch.equal(got, manual) and not torch.equal(got, unguided)


@gpu
def test_cached_loop_with_image_seeds_an_image_equals_its_own_run():
    B = 4
    es, ef = _pair(B)
    ctx, stream = es.ctx, side_stream()
    x0 = images(B, 3, 8, 19)
    seeds = [101, 7, 55, 3]
    plan = _plan("ddpm", 9, 3, 1)
    with ctx.image_seeds(seeds, stream):
        batch = _device(plan, 1, 1, es, ef, x0, stream, noise="philox")
    for i in range(B):
        with ctx.image_seeds(seeds[i:i + 1], stream):
            one = _device(plan, 1, 1, es, ef, x0[i:i + 1].contiguous(), stream, noise="philox")
        assert torch.equal(one[0], batch[i]), f"image {i} differs from its B = 1 run"


@gpu
def test_a_new_cache_setting_is_not_a_stale_graph():
    """(K, N, order) changed one at a time on the same model, and back: each == a freshly built model"""
    B = 4
    x0, stream = images(B, 3, 8, 31), side_stream()
    settings = [(1, 3, 0), (2, 3, 0), (2, 2, 0), (2, 2, 1), (1, 3, 0)]

    def run(em, K, N, order):
        return _device(_plan("ddpm", 8, N, order, late=False, K=K), K, order, em, None, x0, stream, seed=33, noise="philox")

    m, _ = uvit(dict(TINY, depth=5), 43, "bf16", B)
    em = m.engine_model(B)
    got = [run(em, *s) for s in settings]
    fresh = []
    for s in settings[:4]:
        fm, _ = uvit(dict(TINY, depth=5), 43, "bf16", B)
        fresh.append(run(fm.engine_model(B), *s))
        del fm
    fresh.append(fresh[0])
    for i in range(3):
        assert not torch.equal(fresh[i], fresh[i + 1])
    for s, g, f in zip(settings, got, fresh):
        assert torch.equal(g, f), f"{s}: replayed a graph of another setting"


@gpu
@pytest.mark.parametrize("case", ["tiny", "qa512"])
def test_cached_loop_reads_no_stale_workspace_bytes(case):
    """forced chains, both chains' workspaces poisoned (NaN bytes) before the call == fresh models: on the fragment hand-off model the
    seam's skip_linear finds block K - 1's patch rows row-major"""
    cfg_s, cfg_f, B, S, n, K = (dict(TINY, depth=3), dict(TINY, depth=5), 6, 8, 7, 1) if case == "tiny" else \
        (dict(QA512, depth=5), dict(QA512, depth=5), 2, 64, 4, 2)
    x0, stream = images(B, 3, S, 35), side_stream()
    plan = _plan("ddpm", n, 2, 1, t_switch=3, K=K)
    outs = []
    for poison in (False, True):
        es, ef, _ = engine_pair(cfg_s, cfg_f, (71, 72), B)
        ctx = es.ctx
        if poison:
            with torch.cuda.stream(stream):
                for e in (es, ef):
                    ctx.check(ctx.lib.dd_dev_poison_workspaces(ctx.handle, e.handle, stream.cuda_stream))
        outs.append((_device(plan, K, 1, es, ef, x0, stream, seed=37, noise="philox", flags=L.DD_DEV_FORCE_CHAINS),
                     ctx.lib.dd_dev_last_sample_chains(ctx.handle)))
        del es, ef
    assert outs[0][1] == outs[1][1] == 2
    assert torch.isfinite(outs[0][0]).all() and not torch.equal(outs[0][0], x0)
    assert torch.equal(outs[0][0], outs[1][0]), "the cached loop differs after the workspaces were poisoned"


@gpu
def test_invalid_cached_calls_are_rejected_before_anything_is_enqueued():
    """DD_ERR_INVALID with a message, the tensors untouched and no graph captured"""
    from duodiff_amd.engine import Model
    B, n = 4, 3
    es, ef = _pair(B)                                        # depths 3 and 5: h = 1 and 2
    ctx, lib = es.ctx, es.ctx.lib
    ee = Model(ctx, ModelParams.from_dict(dict(TINY, depth=5)), B)
    ee.enable_early_exit("mlp_probe_per_layer")
    x0, stream = images(B, 3, 8, 39), side_stream()
    f = (C.c_float * n)(900.0, 600.0, 300.0)
    one = (C.c_float * n)(1.0, 1.0, 1.0)
    nz = (C.c_int32 * n)(0, 0, 0)
    ops = lambda *v: (C.c_int32 * n)(*v)
    # (first, late, noise mode, (blocks, order, op array, w array) or None, message)
    cases = [(ef, None, L.DD_NOISE_NONE, None, "null dd_block_cache"), (ef, None, L.DD_NOISE_NONE, (1, 0, None, one), "null"),
             (ef, None, L.DD_NOISE_NONE, (1, 0, nz, None), "null"), (ef, None, L.DD_NOISE_NONE, (0, 0, nz, one), "blocks"),
             (ef, None, L.DD_NOISE_NONE, (3, 0, nz, one), "blocks"), (es, ef, L.DD_NOISE_NONE, (2, 0, nz, one), "blocks"),
             (ef, None, L.DD_NOISE_NONE, (1, 2, nz, one), "order"), (ef, None, L.DD_NOISE_NONE, (1, -1, nz, one), "order"),
             (ef, None, L.DD_NOISE_NONE, (1, 1, ops(0, 3, 0), one), "outside {0, 1, 2}"),
             (ef, None, L.DD_NOISE_NONE, (1, 0, ops(0, 0, 2), one), "under order 0"),
             (ef, None, L.DD_NOISE_NONE, (1, 0, ops(1, 0, 0), one), "no refresh"),             # the first row reuses: never refreshed
             (es, ef, L.DD_NOISE_NONE, (1, 0, ops(0, 1, 0), one), "no refresh"),                # ... the late model's first row (switch at 1)
             (ef, None, L.DD_NOISE_NONE, (1, 1, ops(0, 2, 0), one), "no second refresh"),
             (ee, None, L.DD_NOISE_NONE, (1, 0, nz, one), "early-exit"), (ef, None, L.DD_NOISE_BUFFER, (1, 0, nz, one), "noise")]
    n0 = lib.dd_dev_graph_captures(ctx.handle)
    for first, late, noise_mode, bcv, msg in cases:
        for use_graph in (1, 0):
            x = x0.clone()
            a = L.dd_affine_sample_args()
            a.first, a.late, a.n_steps, a.switch_after = first.handle, late.handle if late else None, n, 1
            a.t, a.a, a.b, a.c, a.noise = f, one, one, one, nz
            a.noise_mode, a.use_graph, a.seed, a.y_dev, a.x_dev, a.B = noise_mode, use_graph, 1, None, x.data_ptr(), B
            bc = L.dd_block_cache(bcv[0], bcv[1], bcv[2], bcv[3]) if bcv else None
            with torch.cuda.stream(stream):
                rc = lib.dd_sample_affine_cached(ctx.handle, C.byref(a), None, None, C.byref(bc) if bc else None, C.c_void_p(stream.cuda_stream))
            stream.synchronize()
            err = lib.dd_last_error(ctx.handle).decode()
            assert rc == L.DD_ERR_INVALID, f"{msg}: status {rc}"
            assert msg in err, err
            assert torch.equal(x, x0), f"{msg}: something was enqueued"
    # the single forward
    for blocks, op, w, msg in ((0, 0, 0.0, "blocks"), (3, 0, 0.0, "blocks"), (1, 3, 0.0, "op"), (1, 1, 0.0, "no refresh"), (1, 2, 1.0, "no refresh"),
                               (1, 2, float("nan"), "finite")):
        x, eps = x0.clone(), torch.zeros_like(x0)
        rc = lib.dd_forward_cached(ctx.handle, ef.handle, C.c_void_p(x.data_ptr()), 500.0, None, None, blocks, op, w, C.c_void_p(eps.data_ptr()), B,
                                   C.c_void_p(stream.cuda_stream))
        stream.synchronize()
        assert rc == L.DD_ERR_INVALID and msg in lib.dd_last_error(ctx.handle).decode(), (msg, lib.dd_last_error(ctx.handle).decode())
        assert torch.equal(x, x0) and not eps.any()
    with torch.cuda.stream(stream):
        ef.forward_cached(x0, 500.0, blocks=1, op=0, stream=stream)                       # one refresh: a reuse is fine, no prev yet
        ef.forward_cached(x0, 500.0, blocks=1, op=1, stream=stream)
        with pytest.raises(ValueError, match="no second refresh"):
            ef.forward_cached(x0, 500.0, blocks=1, op=2, w=1.0, stream=stream)
        with pytest.raises(ValueError, match="no refresh"):                            # other blocks, another batch: another geometry
            ef.forward_cached(x0, 500.0, blocks=2, op=1, stream=stream)
        with pytest.raises(ValueError, match="no refresh"):
            ef.forward_cached(x0[:2].contiguous(), 500.0, blocks=1, op=1, stream=stream)
        with pytest.raises(ValueError, match="early-exit"):
            ee.forward_cached(x0, 500.0, blocks=1, op=0, stream=stream)
    stream.synchronize()
    assert lib.dd_dev_graph_captures(ctx.handle) == n0


# ---- GPU, the sampler ------------------------------------------------------------------------------------------------------------
@gpu
def test_get_samples_with_a_cache_runs_every_sampler():
    """get_samples(cache=...) through DDPM (cut short) and DDIM, on a single model and on a pair, device noise and the step-by-step torch_cpu
    path; cache=None is the run without the option, a cache moves the samples, N = 1 on the DDIM rows is the uncached run in fp32"""
    from duodiff_amd import sampler
    ms, _ = uvit(dict(TINY, depth=3), 91, "bf16", None)
    mf, _ = uvit(dict(TINY, depth=5), 92, "bf16", None)
    common = dict(batch_size=3, postprocessing=sampler.predict_noise_postprocessing, seed=3, num_channels=3, sample_height=8, sample_width=8)
    for models in (dict(model=mf), dict(model=ms, late_model=mf, t_switch=4)):
        K = 2 if "late_model" not in models else 1
        for kw in (dict(num_steps=8, timesteps_save=[3, 6]), dict(use_ddim=True, ddim_steps=9)):
            for noise in ("device", "torch_cpu"):
                base, _ = sampler.get_samples(noise=noise, **models, **common, **kw)
                none, _ = sampler.get_samples(noise=noise, cache=None, **models, **common, **kw)
                assert np.array_equal(none, base)
                for order in (0, 1):
                    moved, inter = sampler.get_samples(noise=noise, cache=(K, 3, order), **models, **common, **kw)
                    assert np.isfinite(moved).all() and moved.shape == (3, 8, 8, 3) and len(inter) == len(kw.get("timesteps_save", ()))
                    assert not np.array_equal(moved, base), f"{kw} {noise} order {order}: the option changed nothing"
    with pytest.raises(ValueError, match="depth"):
        sampler.get_samples(ms, late_model=mf, t_switch=4, cache=(2, 3, 0), **common)
    with pytest.raises(ValueError, match="combine"):
        sampler.get_samples(mf, cache=(1, 3, 0), pag=(1.0, [0], [0]), **common)
    with pytest.raises(ValueError, match="combine"):
        sampler.get_samples(ms, late_model=mf, cache=(1, 3, 0), autoguidance_scale=1.0, **common)
    with pytest.raises(ValueError, match="DPM-Solver"):
        sampler.get_samples(mf, cache=(1, 3, 0), solver="dpmsolver++", **common)
    with pytest.raises(ValueError, match="cache_order"):
        sampler.get_samples(mf, cache=(1, 3, 2), **common)


@gpu
def test_get_samples_device_and_host_paths_agree_without_noise():
    """DDIM at eta 0 draws nothing that enters x: the device loop (cut at the saves) and the step-by-step forward_cached path give the same images"""
    from duodiff_amd import sampler
    mf, _ = uvit(dict(TINY, depth=5), 92, "bf16", None)
    common = dict(batch_size=3, postprocessing=sampler.predict_noise_postprocessing, seed=3, num_channels=3, sample_height=8, sample_width=8,
                  use_ddim=True, ddim_steps=9, timesteps_save=[250, 625], cache=(2, 3, 1))
    dev, di = sampler.get_samples(mf, noise="device", **common)
    host, hi = sampler.get_samples(mf, noise="torch_cpu", **common)
    assert np.array_equal(dev, host) and len(di) == len(hi) and all(np.array_equal(a, b) for a, b in zip(di, hi))


@gpu
def test_cli_cache_end_to_end(tmp_path):
    """A synthetic depth-5 checkpoint written here: --cache_blocks 2 writes finite samples of the right shape, which differ from the run
    without the option"""
    import yaml
    cfg = dict(TINY, depth=5, img_size=16)
    (tmp_path / "m.yaml").write_text(yaml.safe_dump({"model_params": cfg}))
    torch.save(dict(synthetic_state_dict(ModelParams.from_dict(cfg), 91)), tmp_path / "m.pth")
    got = {}
    for name, extra in (("cached", ["--cache_blocks", "2", "--cache_order", "1"]), ("off", [])):
        out = tmp_path / f"out{name}"
        cmd = [sys.executable, "-m", "duodiff_amd.sampler", "--seed", "5", "--checkpoint_path", str(tmp_path / "m.pth"),
               "--config_path", str(tmp_path / "m.yaml"), "--batch_size", "3", "--parametrization", "predict_noise",
               "--output_folder", str(out), "--no_png", "--use_ddim", "--ddim_steps", "10", "--noise", "device", *extra]
        r = subprocess.run(cmd, cwd=str(REPO), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        got[name] = np.load(out / "samples.npy")
        assert got[name].shape == (3, 16, 16, 3) and np.isfinite(got[name]).all()
    assert not np.array_equal(got["cached"], got["off"])
