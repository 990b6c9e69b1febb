"""Per-image seeds on the GPU: an image depends on its seed, not on its batch (dd_set_image_seeds, dd_noise_images, dd_dev_final_seeded;
step_update.h draw_site).

The anchor to the behaviour before: a seeded image with seed s draws exactly what the plain call with B = 1 and seed = s draws.  So the
loop tests compare row i of a seeded batch with the PLAIN call on image i alone, bit for bit, and need no reference of their own.
  kernel level   z and z2 of dd_dev_final_seeded per element against kernel_support.philox_normal4_ref (key seeds[b0 + b], ids y S + x) within
                 test_final_step's PHILOX_BOUND -- measured there on this draw function, which is unchanged -- and bit for bit against the plain
                 B = 1 launch; equal seeds give equal images, permuted seeds permuted images; one step with guidance, history and a known
                 region at once as the composition of its own draws; dd_noise_images against the same reference under its own stream word.
  loops          B = 6 with distinct seeds through every loop that draws: row i == the plain B = 1 call, permutation, the chain and graph
                 forms, a cut loop, dd_sample_step.  Each comparison runs with noise="none" first: if that control fails, the backbone
                 is at fault, not the seeds, and the message says so.
  state, errors  set -> clear restores the plain bits; other seeds replay the same graphs; n != B and NULL with n are DD_ERR_INVALID.
  sampler        get_samples(image_seeds=) of 4 == two calls of 2; the command lines (--image_seeds --first_image; two ranks over gloo).
"""
import contextlib
import functools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import kernel_support as ks
import test_final_step as tfs
from conftest import REPO, TINY
from duodiff_amd import _lib as L
from duodiff_amd.config import ModelParams
from duodiff_amd.weights import synthetic_state_dict
from kernel_support import F32
from loop_support import NULL, TINY_COND, ddpm_rows, dev_flags, ee_uvit, images, known_region, run_loop, side_stream, uvit

pytestmark = pytest.mark.gpu

PHILOX_START = 0x78545F30          # step_update.h
BIG = (7 << 32) | 0x9ABCDEF1        # a seed above 2^32
SEEDS = [BIG, 3, (1 << 63) | 0x55, 0x1234, (1 << 32) + 3, 41, 0xDEADBEEF, 7, 99, 12345678901234567]


# ---------------------------------------------------------------------------------------------------------------- the kernel level
@contextlib.contextmanager
def seeded_final(seeds, n=None, null=False):
    """test_final_step.launch / draw through dd_dev_final_seeded: the entry point they call is dd_dev_final with the seeds appended
    (n, null: another count than len(seeds), a null array -- the rejected calls)"""
    lib = ks.ctx().lib
    arr = np.ascontiguousarray(seeds, np.uint64)
    plain = lib.dd_dev_final
    lib.dd_dev_final = lambda h, q, stream: lib.dd_dev_final_seeded(h, q, None if null else arr.ctypes.data, int(arr.size if n is None else n), stream)
    try:
        yield
    finally:
        lib.dd_dev_final = plain


def image_ids(S):
    return ks.final_pixel_ids(1, S, 0)[0]          # y S + x


def seeded_ref(seeds, b0, B, C_, S, ctr, stream):
    """[B, C, S, S] float64: image b under key seeds[b0 + b] with image-local pixel ids"""
    return np.stack([ks.philox_normal4_ref(seeds[b0 + b], image_ids(S), ctr, stream)[0][..., :C_].transpose(2, 0, 1) for b in range(B)])


DRAWS = [dict(S=8, C=3, b0=0, ctr=0, z2=False), dict(S=24, C=4, b0=5, ctr=941, z2=False), dict(S=24, C=1, b0=5, ctr=17, z2=True),
         dict(S=8, C=4, b0=0, ctr=941, z2=True), dict(S=24, C=3, b0=0, ctr=17, z2=False), dict(S=8, C=1, b0=5, ctr=0, z2=False),
         dict(S=24, C=3, b0=5, ctr=941, z2=True)]


@pytest.mark.parametrize("case", DRAWS, ids=lambda c: f"S{c['S']}-C{c['C']}-b{c['b0']}-k{c['ctr']}-{'z2' if c['z2'] else 'z'}")
def test_seeded_draw_against_the_reference_and_the_plain_single_image_launch(case):
    B, b0 = 3, case["b0"]
    seeds = SEEDS[:b0 + B]
    case = dict(case, B=B, seed=0x777)                                     # (the launch's own seed must not matter)
    with seeded_final(seeds):
        got = tfs.draw(case)
    want = seeded_ref(seeds, b0, B, case["C"], case["S"], case["ctr"], ks.PHILOX_KNOWN if case["z2"] else ks.PHILOX_STEP)
    err = np.abs(got - want).max()
    print(f"seeded draw: max |z - ref| {err:.3e} of the bound {tfs.PHILOX_BOUND:.3e}")
    ks.gate(got, want, tfs.PHILOX_BOUND, "seeded z against philox_normal4_ref under the image's seed")
    for b in range(B):                                                     # the B = 1 equivalence, bit for bit
        alone = tfs.draw(dict(case, B=1, b0=0, seed=seeds[b0 + b]))
        assert np.array_equal(got[b].astype(F32).view(np.uint32), alone[0].astype(F32).view(np.uint32)), f"image {b} != the plain B = 1 launch"


def test_seeded_draw_depends_on_the_seed_not_on_the_position():
    case = dict(S=24, C=3, B=3, b0=0, ctr=5, z2=False, seed=1)
    with seeded_final([BIG, 3, BIG]):
        a = tfs.draw(case)
    assert np.array_equal(a[0], a[2]) and not np.array_equal(a[0], a[1])
    with seeded_final([3, BIG, 41]):
        b = tfs.draw(case)
    assert np.array_equal(b[0], a[1]) and np.array_equal(b[1], a[0]) and not np.array_equal(b[2], a[0])
    with seeded_final([9, 9, 9, 9, 9, 3, BIG, 41]):                         # the same images in a launch that starts at image 5
        c = tfs.draw(case, b0=5)
    assert np.array_equal(c, b)


def test_seeded_step_with_guidance_history_and_known_region_is_the_composition_of_its_draws():
    """final_tiled_kernel<3,2,G,H,K> seeded: classifier-free guidance, history and a known region in one launch, bit for bit from the kernel's
    own eps and its own seeded z and z2 (the twin row b + pair_B draws under image b's seed: it receives image b's x'')"""
    seeds = SEEDS[:8]
    case = dict(S=24, B=3, C=3, b0=5, seed=0, ctr=tfs.ROW["ctr"], z2=False)
    with seeded_final(seeds):
        z, z2 = tfs.draw(case).astype(F32), tfs.draw(dict(case, z2=True)).astype(F32)
        a = ks.final_head_inputs(3, 2, 24, "cfg")
        x, _, h, kx0, kmask = tfs.step_operands(a, 9)
        o = tfs.launch(a, write_x=True, x_in=x, h=h, kx0=kx0, kmask=kmask, t=6, seed=0, noise_mode=L.DD_NOISE_PHILOX, row=tfs.ROW,
                       hist=tfs.HIST, known=tfs.KNOWN, b0=5)
    tfs.check_eps(a, o, "seeded step")
    n = 3 * o.img
    eps = o.eps[:n].reshape(z.shape)
    xp = ks.step_table(x[:3], eps, z, h[:n].reshape(z.shape), tfs.ROW["a"], tfs.ROW["b"], tfs.ROW["c"], tfs.HIST["d"], 1)
    xp = ks.step_known(xp, kx0, np.broadcast_to(kmask, xp.shape), tfs.KNOWN["ka"], tfs.KNOWN["kb"], z2)
    assert np.array_equal(o.x[:n].view(np.uint32), xp.reshape(-1).view(np.uint32))
    assert np.array_equal(o.x[n:2 * n].view(np.uint32), o.x[:n].view(np.uint32)) and ks.untouched(o.x[2 * n:])
    # autoguidance (the other guided instantiation) draws the same z: x' differs from a launch under other seeds, and only by c (z - z')
    g = ks.final_head_inputs(3, 2, 24, "auto")
    xg, _, _, _, _ = tfs.step_operands(g, 9)
    outs = []
    for sd in (seeds, seeds[::-1]):
        with seeded_final(sd):
            outs.append(tfs.launch(g, write_x=True, x_in=xg, t=6, noise_mode=L.DD_NOISE_PHILOX, row=tfs.ROW, b0=5))
    zr = seeded_ref(seeds[::-1], 5, 3, 3, 24, tfs.ROW["ctr"], ks.PHILOX_STEP)
    diff = (outs[0].x[:n].astype(np.float64) - outs[1].x[:n]).reshape(z.shape)
    assert np.abs(diff - tfs.ROW["c"] * (z.astype(np.float64) - zr)).max() < 5e-5         # (fp32 roundings of x'; a wrong seed is an error of order 1)


def test_final_seeded_rejects_bad_seed_arrays():
    a = ks.final_head_inputs(3, 4, 16)
    x, z, _, _, _ = tfs.step_operands(a, 1)
    ok = dict(write_x=True, x_in=x, z=z, t=3, noise_mode=L.DD_NOISE_PHILOX, ddpm=tfs.DDPM, b0=2)
    for bad in (dict(null=True), dict(n=0), dict(n=-1), dict(n=4), dict(n=(1 << 22) + 1)):          # (n = 4 < b0 + B = 5)
        with seeded_final(np.arange(8), **bad):
            o = tfs.launch(a, expect=L.DD_ERR_INVALID, **ok)
        assert np.all(o.eps == 0) and np.all(o.x == 0) and o.q.t_out == -12345, bad
    with seeded_final(np.arange(8), n=5):
        tfs.launch(a, **ok)


# ---------------------------------------------------------------------------------------------------------------- dd_noise_images
def noise_images(B, C_, S, seed=0, seeds=None, counter=0, expect=L.DD_OK, misalign=0, over=()):
    """dd_noise_images into a buffer with eight canary floats behind the end (misalign: the output starts that many floats into it;
    over: arguments of the call replaced by name -- the rejected calls)"""
    ctx = ks.ctx()
    n = B * C_ * S * S
    buf = torch.full((misalign + n + 8,), float("nan"), device="cuda")
    buf.view(torch.int32).fill_(-1)
    sd = None if seeds is None else torch.from_numpy(np.array(seeds, np.uint64).view(np.int64)).cuda()
    a = dict(B=B, C=C_, S=S, counter=counter, out=buf.data_ptr() + 4 * misalign)
    a.update(dict(over))
    torch.cuda.synchronize()
    rc = ctx.lib.dd_noise_images(ctx.handle, seed, None if sd is None else sd.data_ptr(), a["counter"], a["out"], a["B"], a["C"], a["S"], None)
    torch.cuda.synchronize()
    assert rc == expect, (rc, ctx.lib.dd_last_error(ctx.handle))
    host = buf.cpu().numpy()
    return host[misalign:misalign + n].reshape(B, C_, S, S), host[misalign + n:], host[:misalign]


@pytest.mark.parametrize("B,C_,S", [(3, 3, 24), (2, 4, 8), (3, 1, 5)])       # (S = 5: 25 pixels per image, the plain-store path)
@pytest.mark.parametrize("counter", [0, 3])
def test_noise_images_plain_and_seeded(B, C_, S, counter):
    got, canary, _ = noise_images(B, C_, S, seed=BIG, counter=counter)
    want, _ = ks.philox_normal4_ref(BIG, ks.final_pixel_ids(B, S, 0), counter, PHILOX_START)
    ks.gate(got, want[..., :C_].transpose(0, 3, 1, 2), tfs.PHILOX_BOUND, "plain x_T")
    assert ks.untouched(canary)
    seeds = SEEDS[:B]
    got_s, canary, _ = noise_images(B, C_, S, seed=5, seeds=seeds, counter=counter)
    ks.gate(got_s, seeded_ref(seeds, 0, B, C_, S, counter, PHILOX_START), tfs.PHILOX_BOUND, "seeded x_T")
    assert ks.untouched(canary)
    for b in range(B):
        alone, _, _ = noise_images(1, C_, S, seed=seeds[b], counter=counter)
        assert np.array_equal(got_s[b].view(np.uint32), alone[0].view(np.uint32)), f"image {b} != the plain B = 1 call under its seed"


def test_noise_images_unaligned_output_takes_plain_stores():
    want, _, _ = noise_images(2, 3, 8, seed=9)
    got, canary, front = noise_images(2, 3, 8, seed=9, misalign=1)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and ks.untouched(canary) and ks.untouched(front)


def test_noise_images_is_independent_of_the_step_noise():
    """the same key, pixel ids and counter: x_T differs from the step's z and the known region's z2 (its own stream word)"""
    xT, _, _ = noise_images(3, 3, 24, seed=0x1234, counter=17)
    case = dict(S=24, B=3, C=3, b0=0, seed=0x1234, ctr=17, z2=False)
    z, z2 = tfs.draw(case), tfs.draw(dict(case, z2=True))
    for other in (z, z2):
        assert (xT != other).mean() > 0.999
        assert abs(np.corrcoef(xT.ravel(), other.ravel())[0, 1]) < 0.1
    got, _, _ = noise_images(3, 3, 24, seed=0x1234, seeds=SEEDS[:3], counter=17)
    assert not np.array_equal(got, xT)


def test_noise_images_rejects_bad_arguments():
    for over in (dict(C=0), dict(C=5), dict(S=0), dict(S=-3), dict(B=-1), dict(counter=-1), dict(out=None), dict(S=32769)):
        got, canary, _ = noise_images(2, 3, 8, expect=L.DD_ERR_INVALID, over=over)
        assert ks.untouched(got) and ks.untouched(canary), over
    ctx = ks.ctx()
    assert ctx.lib.dd_noise_images(None, 0, None, 0, None, 1, 1, 1, None) == L.DD_ERR_INVALID
    got, canary, _ = noise_images(2, 3, 8, over=dict(B=0))                              # nothing to do
    assert ks.untouched(got)


def test_context_noise_images_wrapper():
    ctx = ks.ctx()
    x = ctx.noise_images(4, 3, 8, image_seeds=SEEDS[:4])
    for i in range(4):
        assert torch.equal(x[i:i + 1], ctx.noise_images(1, 3, 8, seed=SEEDS[i]))
        assert torch.equal(x[i:i + 1], ctx.noise_images(1, 3, 8, image_seeds=[SEEDS[i]]))
    with pytest.raises(ValueError):
        ctx.noise_images(4, 3, 8, image_seeds=SEEDS[:3])


# ---------------------------------------------------------------------------------------------------------------- the loops
B6, CFG = 6, TINY_COND
KINDS = ["ddpm_switch", "affine_eta", "multistep_sde", "threshold", "region", "guided", "autoguided", "perturbed", "early_exit"]


class Models:
    pass


@pytest.fixture(scope="module")
def M():
    """one set of models for every loop test (max_batch 12: the 2 B backbone rows of either row-doubling guidance at B = 6)"""
    m = Models()
    m.first = uvit(dict(CFG, depth=1), 31, "bf16", 12)[0].engine_model(12)
    m.late = uvit(dict(CFG, depth=3), 32, "bf16", 12)[0].engine_model(12)
    m.ee_module = ee_uvit(dict(CFG), 33, "mlp_probe_per_layer", "bf16", 12)[0]
    m.ee = m.ee_module.engine_model(12)
    g = torch.Generator().manual_seed(77)
    m.x = torch.randn(B6, 3, 8, 8, generator=g).cuda()
    m.y = torch.tensor([1, 7, 3, 0, 9, 4]).cuda()
    m.x0 = torch.randn(B6, 3, 8, 8, generator=g).cuda()
    i = torch.arange(8)
    mask = ((i[:, None] + i[None, :]) % 2).float().expand(B6, 1, 8, 8).clone()
    mask[:, :, 1::3, ::2] = 0.5
    for b in range(B6):
        mask[b] = torch.roll(mask[b], b, -1)                                 # (the images' masks differ)
    m.mask = mask.cuda()
    _, cls0, _ = m.ee_module(m.x.cpu(), torch.full((B6,), 5.0), m.y.cpu())
    m.ee_thr = float(torch.stack(cls0)[0].median())                          # about half of the images leave at the first layer
    m.stream = side_stream()
    return m


@functools.lru_cache(maxsize=None)
def plans():
    from duodiff_amd import sampler
    from duodiff_amd.engine import X0Threshold
    thr = X0Threshold("dynamic", 0.9, s_max=4.0)
    return dict(
        affine=sampler.step_plan(None, use_ddim=True, ddim_steps=7, ddim_eta=0.01),
        multistep=sampler.step_plan("predict_noise", solver="sde-dpmsolver++", solver_steps=6),
        threshold=(sampler.step_plan("predict_noise", solver="sde-dpmsolver++", solver_steps=6, threshold=thr), thr),
        region=sampler.step_plan("predict_noise", strength=5 / 999))


def run(kind, M, idx, *, seeds=None, seed=0, noise="philox", flags=0, use_graph=True, cut=None):
    """loop `kind` on the images idx of the module's batch (x, y, known image and mask), seeded (seeds: one per image of idx) or plain under
    `seed`; cut: the loop in two calls, the second from step `cut` on (counter base / timestep and h carried) -> x"""
    from duodiff_amd import engine
    ctx, st = M.late.ctx, M.stream
    idx = list(idx)
    x_in, y = M.x[idx], M.y[idx].clone()
    kw = dict(y=y, seed=seed, noise=noise, use_graph=use_graph, flags=flags, image_seeds=seeds, cuts=() if cut is None else (cut,))
    if kind == "early_exit":                                                 # the one entry run_loop does not drive
        x, n = x_in.clone(), 10
        with dev_flags(ctx, flags), torch.cuda.stream(st), ctx.image_seeds(seeds, st):
            for k0, k1 in zip([0, *kw["cuts"]], [*kw["cuts"], n]):
                engine.sample_early_exit_loop(ctx, M.ee, x, M.ee_thr, t_start=n - 1 - k0, t_end=n - k1, y=y, seed=seed, noise=noise,
                                              use_graph=use_graph, stream=st)
            st.synchronize()
            chains = ctx.lib.dd_dev_last_sample_chains(ctx.handle)
    elif kind == "ddpm_switch":                                              # the late model takes over behind t = 5
        x, _, chains = run_loop("ddpm", M.first, x_in, ddpm_rows(10, 9), st, late=M.late, t_switch=995, **kw)
    elif kind in ("guided", "perturbed"):
        g = (0.4, NULL) if kind == "guided" else engine.Perturbed(0.5, [1])
        x, _, chains = run_loop("ddpm", M.late, x_in, ddpm_rows(6, 5), st, guidance=g, **kw)
    elif kind == "region":
        plan = plans()["region"]
        assert (known_region(plan, None, None, 0, cut).kb != 0).any(), "the region's rows must draw z2"
        x, _, chains = run_loop("ddpm", M.late, x_in, plan, st, region=(M.x0[idx].clone(), M.mask[idx].clone()), **kw)
    else:
        plan, thr = plans()["threshold"] if kind == "threshold" else (plans()["multistep" if kind == "multistep_sde" else "affine"], None)
        assert kind == "threshold" or plan.rows["noise"][:cut].any()
        g = engine.Autoguidance(M.first, 0.7) if kind == "autoguided" else None
        x, _, chains = run_loop("affine" if kind in ("affine_eta", "autoguided") else "multistep", M.late, x_in, plan, st, threshold=thr,
                                guidance=g, **kw)
    assert flags != L.DD_DEV_FORCE_CHAINS or chains == 2
    assert bool(torch.isfinite(x).all())
    return x


def both(what, a, b):
    """a(noise) == b(noise), first without noise (the control), then with the device noise"""
    assert torch.equal(a("none"), b("none")), f"{what}: the control WITHOUT noise differs -- the backbone is at fault, not the per-image seeds"
    ga, gb = a("philox"), b("philox")
    assert torch.equal(ga, gb), f"{what}: differs with the device noise in {(ga != gb).any(dim=(1, 2, 3)).tolist()} (per image)"
    return ga


@pytest.mark.parametrize("kind", KINDS)
def test_seeded_loop(kind, M):
    seeds, every = SEEDS[:B6], range(B6)
    cache = {}

    def whole(noise):
        if noise not in cache:
            cache[noise] = run(kind, M, every, seeds=seeds, noise=noise)
        return cache[noise]

    assert not torch.equal(whole("philox"), whole("none")), "the loop must draw"
    # 1. row i == today's plain call on image i alone under its seed
    for i in every:
        both(f"{kind}: image {i} against the plain B = 1 call", lambda nz: whole(nz)[i:i + 1], lambda nz: run(kind, M, [i], seed=seeds[i], noise=nz))
    # (and the plain batch is not that: its image 1 depends on its position)
    assert not torch.equal(run(kind, M, every, seed=seeds[1])[1:2], whole("philox")[1:2])
    # 2. a permutation of the images and their seeds permutes the result
    perm = [4, 0, 5, 2, 1, 3]
    both(f"{kind}: permuted", lambda nz: whole(nz)[perm], lambda nz: run(kind, M, perm, seeds=[seeds[p] for p in perm], noise=nz))
    # 3. two half-batch chains, one chain, eager launches
    for name, form in (("two chains", dict(flags=L.DD_DEV_FORCE_CHAINS)), ("one chain", dict(flags=L.DD_DEV_NO_CHAINS)), ("eager", dict(use_graph=False))):
        both(f"{kind}: {name}", whole, lambda nz: run(kind, M, every, seeds=seeds, noise=nz, **form))
    # 4. the loop cut in two
    both(f"{kind}: cut after step 3", whole, lambda nz: run(kind, M, every, seeds=seeds, noise=nz, cut=3, flags=L.DD_DEV_FORCE_CHAINS))


def test_sample_step_driven_step_by_step_equals_the_loop(M):
    from duodiff_amd import engine
    ctx, st, seeds = M.late.ctx, M.stream, SEEDS[:B6]
    for noise in ("none", "philox"):
        want = M.x.clone()
        with torch.cuda.stream(st), ctx.image_seeds(seeds, st):
            engine.sample_loop(ctx, M.late, None, want, t_start=7, t_end=0, y=M.y, seed=123, noise=noise, stream=st)
        got = M.x.clone()
        with torch.cuda.stream(st), ctx.image_seeds(seeds, st):
            for t in range(7, -1, -1):
                M.late.sample_step(got, t, y=M.y, noise=noise, seed=456, stream=st)
        st.synchronize()
        assert torch.equal(got, want), "control without noise: the backbone is at fault" if noise == "none" else "dd_sample_step under per-image seeds"
    # DD_NOISE_BUFFER steps are what they are without the seeds
    z = images(B6, 3, 8, 3)
    a, b = M.x.clone(), M.x.clone()
    with torch.cuda.stream(st):
        M.late.sample_step(a, 5, y=M.y, z=z, noise="buffer", stream=st)
        with ctx.image_seeds(seeds[:2], st):                                 # (not even their count matters)
            M.late.sample_step(b, 5, y=M.y, z=z, noise="buffer", stream=st)
    st.synchronize()
    assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- state and errors
def test_set_then_clear_restores_the_plain_loop_and_other_seeds_replay_the_graphs(M):
    ctx = M.late.ctx
    captures = lambda: ctx.lib.dd_dev_graph_captures(ctx.handle)
    before = run("affine_eta", M, range(B6), seed=5)
    a = run("affine_eta", M, range(B6), seeds=SEEDS[:B6], seed=5)
    n = captures()
    b = run("affine_eta", M, range(B6), seeds=SEEDS[1:B6 + 1], seed=5)
    assert captures() == n, "a second seeded call with other seeds must replay the captured step"
    assert not torch.equal(a, b)
    after = run("affine_eta", M, range(B6), seed=5)
    assert torch.equal(before, after) and not torch.equal(before, a)
    assert captures() > n, "switching the mode re-captures (the staged pointer is part of the key)"


def test_wrong_seed_count_is_rejected_before_anything_is_enqueued(M):
    from duodiff_amd import engine
    ctx, st = M.late.ctx, M.stream
    x = M.x.clone()
    calls = {
        "dd_sample": lambda: engine.sample_loop(ctx, M.late, None, x, t_start=3, t_end=0, y=M.y, stream=st),
        "dd_sample_affine": lambda: engine.sample_affine_loop(ctx, M.late, None, x, [500.0], [1.0], [0.5], [1.0], [1], y=M.y, stream=st),
        "dd_sample_early_exit": lambda: engine.sample_early_exit_loop(ctx, M.ee, x, 0.5, t_start=3, t_end=0, y=M.y, stream=st),
        "dd_sample_step": lambda: M.late.sample_step(x, 3, y=M.y, noise="philox", stream=st),
    }
    for name, call in calls.items():
        with torch.cuda.stream(st), ctx.image_seeds(SEEDS[:B6 - 1], st):
            with pytest.raises(ValueError, match="5 seeds.*6 images"):
                call()
        st.synchronize()
        assert torch.equal(x, M.x), f"{name}: x touched by a rejected call"
    with torch.cuda.stream(st), ctx.image_seeds(SEEDS[:B6 - 1], st):         # no device noise: the seeds are not consulted
        engine.sample_loop(ctx, M.late, None, x, t_start=1, t_end=0, y=M.y, noise="none", stream=st)
    st.synchronize()
    assert ctx.lib.dd_set_image_seeds(ctx.handle, None, 3) == L.DD_ERR_INVALID
    assert b"dd_set_image_seeds" in ctx.lib.dd_last_error(ctx.handle)
    sd = torch.zeros(3, dtype=torch.int64, device="cuda")
    assert ctx.lib.dd_set_image_seeds(ctx.handle, sd.data_ptr(), 0) == L.DD_ERR_INVALID
    assert ctx.lib.dd_set_image_seeds(ctx.handle, sd.data_ptr(), -1) == L.DD_ERR_INVALID
    assert ctx.lib.dd_set_image_seeds(None, None, 0) == L.DD_ERR_INVALID
    assert ctx.lib.dd_set_image_seeds(ctx.handle, None, 0) == L.DD_OK
    with pytest.raises(ValueError):
        ctx.set_image_seeds([1 << 64])
    with pytest.raises(ValueError):
        ctx.set_image_seeds([])


# ---------------------------------------------------------------------------------------------------------------- sampler, CLI, dist
PAIR = (dict(TINY, depth=1), dict(TINY, depth=3))


@pytest.mark.parametrize("sampler_kw", [dict(t_switch=5, num_steps=8), dict(solver="sde-dpmsolver++", solver_steps=6, t_switch=400)], ids=["ddpm_switch", "sde"])
def test_get_samples_of_four_is_two_calls_of_two(sampler_kw):
    from duodiff_amd import sampler
    m_s, m_f = uvit(PAIR[0], 21, "bf16", 4)[0], uvit(PAIR[1], 22, "bf16", 4)[0]
    seeds = [11, BIG, 13, 11 + (1 << 40)]
    kw = dict(model=m_s, late_model=m_f, postprocessing=sampler.predict_noise_postprocessing, seed=0, num_channels=3, sample_height=8,
              sample_width=8, noise="device", **sampler_kw)
    whole, _ = sampler.get_samples(batch_size=4, image_seeds=seeds, **kw)
    halves = [sampler.get_samples(batch_size=2, image_seeds=seeds[i:i + 2], **kw)[0] for i in (0, 2)]
    assert np.isfinite(whole).all() and np.array_equal(whole, np.concatenate(halves))
    other, _ = sampler.get_samples(batch_size=4, image_seeds=seeds, **dict(kw, seed=99))
    assert np.array_equal(other, whole), "with image seeds the call's seed is unused"
    plain, _ = sampler.get_samples(batch_size=4, **kw)
    assert not np.array_equal(plain, whole)
    with pytest.raises(ValueError, match="noise"):
        sampler.get_samples(batch_size=4, image_seeds=seeds, **dict(kw, noise="torch_cpu"))
    with pytest.raises(ValueError, match="seeds"):
        sampler.get_samples(batch_size=4, image_seeds=seeds[:3], **kw)


def _files(tmp_path):
    import yaml
    for name, cfg, seed in (("s", PAIR[0], 21), ("f", PAIR[1], 22)):
        (tmp_path / f"{name}.yaml").write_text(yaml.safe_dump({"model_params": dict(cfg)}))
        torch.save(dict(synthetic_state_dict(ModelParams.from_dict(cfg), seed)), tmp_path / f"{name}.pth")


def _argv(tmp_path, module, out, batch_size, *extra):
    return [sys.executable, "-m", module, "--seed", "11", "--checkpoint_path", str(tmp_path / "s.pth"), "--checkpoint_path_late",
            str(tmp_path / "f.pth"), "--config_path", str(tmp_path / "s.yaml"), "--config_path_late", str(tmp_path / "f.yaml"), "--t_switch", "300",
            "--batch_size", str(batch_size), "--parametrization", "predict_noise", "--output_folder", str(out), "--no_png", "--noise", "device",
            "--dpm_solver", "sde", "--dpm_solver_steps", "8", "--image_seeds", *extra]


def test_cli_first_image_regenerates_a_slice_of_the_run(tmp_path):
    _files(tmp_path)
    for out, bs, extra in (("whole", 4, ()), ("slice", 2, ("--first_image", "2"))):
        r = subprocess.run(_argv(tmp_path, "duodiff_amd.sampler", tmp_path / out, bs, *extra), cwd=str(REPO), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
    whole, part = np.load(tmp_path / "whole" / "samples.npy"), np.load(tmp_path / "slice" / "samples.npy")
    assert whole.shape == (4, 8, 8, 3) and np.isfinite(whole).all() and np.array_equal(part, whole[2:4])
    assert not np.array_equal(whole[0], whole[1])


def test_two_ranks_with_image_seeds_equal_one_rank_of_twice_the_batch(tmp_path):
    """two fresh processes as ranks 0 / 1 over gloo on this GPU, then one single-process run of 2 B images: the gathered array is that run"""
    _files(tmp_path)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    B = 2
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   DUODIFF_DIST_BACKEND="gloo")
        procs.append(subprocess.Popen(_argv(tmp_path, "duodiff_amd.dist", tmp_path / "two", B), cwd=str(REPO), env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    for p in procs:
        so, se = p.communicate(timeout=300)
        assert p.returncode == 0, se[-2000:]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run(_argv(tmp_path, "duodiff_amd.dist", tmp_path / "one", 2 * B), cwd=str(REPO), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got, want = np.load(tmp_path / "two" / "samples.npy"), np.load(tmp_path / "one" / "samples.npy")
    assert got.shape == (2 * B, 8, 8, 3) and np.isfinite(got).all()
    assert np.array_equal(got, want), "the gathered shards of two ranks differ from one rank's run of all the images"
