"""The denoising-error scan as a device-resident loop (dd_scan_error through engine.scan_error_loop), on the GPU: bit-equal to its manual
composition from the dev entries and dd_forward, graph replay against eager launches, two chains against one, graph reuse and staleness,
the sampling loops around it unchanged, poisoned workspaces, the errors against the numpy oracle fed the kernel's own x_t, every rejection,
and the command line end to end.  (The early-exit form of the scan is not part of this version.)"""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import kernel_support as ks
from conftest import TINY
from duodiff_amd import _lib as L
from duodiff_amd import step_plan
from duodiff_amd.config import ModelParams
from duodiff_amd.weights import synthetic_state_dict
from kernel_support import F32
from loop_support import QA512, TINY_COND, dev_flags, eps_rms_bound, images, labels, side_stream, uvit
from scan_support import _images, diffuse, draw, error
from scan_support import _scan as _scan_loop

pytestmark = pytest.mark.gpu

GRID = [999, 500, 1, 0]
CASES = {"tiny": (TINY, 5), "tiny_classes": (TINY_COND, 5), "qa512": (QA512, 2)}
PARS = ("predict_noise", "predict_original", "predict_previous")


def _scan(*args, **kw):
    from duodiff_amd.engine import scan_error_loop
    return _scan_loop(scan_error_loop, *args, **kw)


def _manual(em, x0, rows, y, seed, counter_base=0, seeds=None):
    """dev diffuse -> dd_forward -> dev error, step by step: (err [n, B], x_t [n, B, C, S, S], eps [n, ...]) as numpy"""
    x0h = x0.cpu().numpy()
    B = x0h.shape[0]
    errs, xts, epss = [], [], []
    for k in range(len(rows["t"])):
        kw = dict(ka=rows["ka"][k], kb=rows["kb"][k], ctr=counter_base + k, seed=seed, seeds=seeds)
        xt = diffuse(x0h, 0, B, **kw)[0]
        eps = em.forward(torch.from_numpy(xt).cuda(), float(rows["t"][k]), y).cpu().numpy()
        errs.append(error(x0h, eps, 0, B, (rows["tz"][k], rows["t0"][k], rows["tx"][k]), **kw)[0])
        xts.append(xt)
        epss.append(eps)
    return np.stack(errs), np.stack(xts), np.stack(epss)


@pytest.mark.parametrize("case", sorted(CASES))
def test_loop_equals_manual_composition_and_graph_equals_eager(case):
    cfg, B = CASES[case]
    m, mp = uvit(cfg, 11, "bf16", B)
    em = m.engine_model(B)
    x0, y = _images(B, mp, 12)
    for par in PARS if case == "tiny" else ("predict_previous",):
        rows = step_plan.scan_rows(GRID, par)
        want = _manual(em, x0, rows, y, seed=77, counter_base=8)[0]
        eager = _scan(em, x0, rows, y, seed=77, counter_base=8, use_graph=False)
        graph = _scan(em, x0, rows, y, seed=77, counter_base=8, use_graph=True)
        assert np.isfinite(want).all() and (want > 0).all()
        assert np.array_equal(eager, want), f"{case} {par}: the eager loop differs from diffuse -> dd_forward -> error"
        assert np.array_equal(graph, eager), f"{case} {par}: graph replay differs from the eager launches"
    assert not np.array_equal(_scan(em, x0, rows, y, seed=77, counter_base=9), graph)        # other counters: other z


def test_image_seeds_an_image_does_not_depend_on_its_batch():
    B = 6
    em = uvit(TINY, 13, "bf16", B)[0].engine_model(B)
    x0, _ = _images(B, ModelParams.from_dict(TINY), 14)
    rows = step_plan.scan_rows(GRID, "predict_noise")
    seeds = [1000 + 7 * i for i in range(B)]
    with em.ctx.image_seeds(seeds):
        whole = _scan(em, x0, rows, seed=1)
        again = _scan(em, x0, rows, seed=2)                              # the call's own seed is unused
    want = _manual(em, x0, rows, None, seed=0, seeds=np.array(seeds, np.uint64))[0]
    assert np.array_equal(whole, want) and np.array_equal(again, whole)
    with em.ctx.image_seeds(seeds[2:5]):
        part = _scan(em, x0[2:5].contiguous(), rows)
    assert np.array_equal(part, whole[:, 2:5]), "an image's errors depend on the batch it ran in"
    assert not np.array_equal(_scan(em, x0, rows, seed=1), whole)       # without the seeds: the plain draw


def test_two_chains_equal_one():
    B = 4
    em = uvit(TINY, 15, "bf16", B)[0].engine_model(B)
    ctx = em.ctx
    x0, _ = _images(B, ModelParams.from_dict(TINY), 16)
    rows = step_plan.scan_rows(GRID, "predict_previous")
    outs = {}
    for name, flags in (("chained", L.DD_DEV_FORCE_CHAINS), ("single", L.DD_DEV_NO_CHAINS)):
        with dev_flags(ctx, flags):
            outs[name] = (_scan(em, x0, rows, seed=5), ctx.lib.dd_dev_last_sample_chains(ctx.handle))
    assert outs["chained"][1] == 2 and outs["single"][1] == 1
    assert np.isfinite(outs["single"][0]).all()
    assert np.array_equal(outs["chained"][0], outs["single"][0]), "the two half-batch chains differ from the single chain"
    # chain 0 of two (2 images from image 0, err rows of 4) is not the whole batch's captured step of 2 images
    with dev_flags(ctx, L.DD_DEV_NO_CHAINS):
        half = _scan(em, x0[:2].contiguous(), rows, seed=5)
    with dev_flags(ctx, L.DD_DEV_FORCE_CHAINS):
        both = _scan(em, x0, rows, seed=5)
    with dev_flags(ctx, L.DD_DEV_NO_CHAINS):
        assert np.array_equal(_scan(em, x0[:2].contiguous(), rows, seed=5), half)
    assert np.array_equal(both, outs["single"][0]) and np.array_equal(half, both[:, :2])


def test_graph_reuse_and_no_stale_graph():
    """other tensors of the same shape replay the captured step; another table, target or counter base is honoured by the replay"""
    B = 3
    em = uvit(TINY, 17, "bf16", B)[0].engine_model(B)
    ctx, mp = em.ctx, ModelParams.from_dict(TINY)
    rows = step_plan.scan_rows(GRID, "predict_noise")
    xa, _ = _images(B, mp, 18)
    xb, _ = _images(B, mp, 19)
    stream = side_stream()
    first = _scan(em, xa, rows, seed=3, stream=stream)
    n0 = ctx.lib.dd_dev_graph_captures(ctx.handle)
    second = _scan(em, xb, rows, seed=3, stream=stream, err=torch.full((len(GRID), B), -1.0, device="cuda"))
    assert ctx.lib.dd_dev_graph_captures(ctx.handle) == n0, "a second call with other tensors of the same shape captured again"
    assert np.array_equal(second, _scan(em, xb, rows, seed=3, use_graph=False)) and not np.array_equal(second, first)
    for other in (step_plan.scan_rows([900, 600, 300, 7], "predict_noise"), step_plan.scan_rows(GRID, "predict_original"),
                  step_plan.scan_rows(GRID, "predict_previous"), step_plan.scan_rows(GRID[:3], "predict_noise")):
        got = _scan(em, xa, other, seed=3, stream=stream)
        assert np.array_equal(got, _scan(em, xa, other, seed=3, use_graph=False)), "replayed the step of another table or target"
        assert got.shape != first.shape or not np.array_equal(got, first)
    assert ctx.lib.dd_dev_graph_captures(ctx.handle) == n0               # the rows live in a device table: none of these captured again
    assert np.array_equal(_scan(em, xa, rows, seed=3, stream=stream), first)


def test_sampling_loops_around_a_scan_are_unchanged():
    """a sampling loop (and a region loop, whose staged known image shares the scan's x0 stage) before and after a scan: bit for bit"""
    from duodiff_amd.engine import KnownRegion, sample_loop, sample_region_loop
    B = 4
    em = uvit(TINY, 21, "bf16", B)[0].engine_model(B)
    ctx, mp = em.ctx, ModelParams.from_dict(TINY)
    xT = images(B, 3, 8, 22)
    x0, _ = _images(B, mp, 23)
    mask = (torch.rand(B, 1, 8, 8, generator=torch.Generator().manual_seed(24)) < 0.5).float().cuda()
    n = 5
    region = KnownRegion(x0, mask, np.linspace(0.2, 1.0, n).astype(F32), np.linspace(0.9, 0.0, n).astype(F32))
    stream = side_stream()

    def sample(fn, *extra):
        x = xT.clone()
        with torch.cuda.stream(stream):
            fn(ctx, em, None, x, *extra, t_start=999, t_end=1000 - n, seed=9, stream=stream)
        stream.synchronize()
        return x

    before = sample(sample_loop), sample(sample_region_loop, region)
    scanned = _scan(em, x0, step_plan.scan_rows(GRID, "predict_noise"), seed=9, stream=stream)
    after = sample(sample_loop), sample(sample_region_loop, region)
    assert np.isfinite(scanned).all() and torch.isfinite(before[0]).all()
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1]), "a scan changed the sampling loop that follows it"
    assert np.array_equal(_scan(em, x0, step_plan.scan_rows(GRID, "predict_noise"), seed=9, stream=stream), scanned)


@pytest.mark.parametrize("case", ["tiny", "qa512"])
def test_scan_reads_no_stale_workspace_bytes(case):
    cfg, B = (TINY, 4) if case == "tiny" else (QA512, 2)
    x0, _ = _images(B, ModelParams.from_dict(cfg), 25)
    rows = step_plan.scan_rows(GRID[:3], "predict_previous")
    outs = []
    for poison in (False, True):
        em = uvit(cfg, 26, "bf16", B)[0].engine_model(B)
        ctx, stream = em.ctx, side_stream()
        with dev_flags(ctx, L.DD_DEV_FORCE_CHAINS):
            if poison:
                with torch.cuda.stream(stream):
                    ctx.check(ctx.lib.dd_dev_poison_workspaces(ctx.handle, em.handle, stream.cuda_stream))
            outs.append(_scan(em, x0, rows, seed=4, stream=stream))
            assert ctx.lib.dd_dev_last_sample_chains(ctx.handle) == 2
        del em
    assert np.isfinite(outs[0]).all() and np.array_equal(outs[0], outs[1]), "the scan differs after the workspaces were poisoned"


@pytest.mark.parametrize("case", sorted(CASES))
def test_errors_against_the_oracle(case):
    """The oracle (float64 numpy) is fed the kernel's own x_t; the loss is taken in float64 from the kernel's own z.  With d the oracle's
    residual and e the engine's error in the model output, |mean((d + e)^2) - mean(d^2)| <= 2 rms(e) sqrt(err) + rms(e)^2 (Cauchy-Schwarz).
    fp32 engine: |e| <= delta = 1e-4 elementwise, the forward bound the suite already uses.  bf16 engine: rms(e) <= delta =
    eps_rms_bound(depth) sigma(ref), the suite's error model."""
    import oracle
    cfg, B = CASES[case]
    mp = ModelParams.from_dict(cfg)
    sd = synthetic_state_dict(mp, 31)
    orc = oracle.UViTOracle(mp.as_dict(), {k: v.numpy() for k, v in sd.items()})
    x0, y = _images(B, mp, 32)
    x0h, yh = x0.cpu().numpy(), None if y is None else y.cpu().numpy()
    Cn, S = mp.in_chans, mp.img_size
    for par in PARS if case == "tiny" else ("predict_noise",):
        rows = step_plan.scan_rows(GRID, par)
        want, refs = [], []
        for k, t in enumerate(GRID):                                      # the reference, once for both precisions
            z = draw(B, Cn, S, 0, B, ctr=k, seed=55).astype(np.float64)
            xt = diffuse(x0h, 0, B, ka=rows["ka"][k], kb=rows["kb"][k], ctr=k, seed=55)[0]
            ref = orc(xt, np.full((B,), t, np.float32), yh).astype(np.float64)
            tgt = float(rows["tz"][k]) * z + float(rows["t0"][k]) * x0h.astype(np.float64) + float(rows["tx"][k]) * xt.astype(np.float64)
            want.append(((ref - tgt) ** 2).mean((1, 2, 3)))
            refs.append(ref)
        want = np.stack(want)
        for prec in ("fp32", "bf16"):
            em = uvit(cfg, 31, prec, B)[0].engine_model(B)
            got = _scan(em, x0, rows, y, seed=55).astype(np.float64)
            delta = np.full(len(GRID), 1e-4) if prec == "fp32" else np.array([eps_rms_bound(mp.depth) * r.std() for r in refs])
            bound = 2 * delta[:, None] * np.sqrt(want) + delta[:, None] ** 2
            ratio = ks.gate(got, want, bound, f"{case} {par} {prec}: err against the oracle")
            print(f"{case} {par} {prec}: err {want.mean(1).round(4).tolist()} observed / bound {ratio:.3f}")
            del em


def test_invalid_calls_are_rejected_before_anything_is_enqueued():
    from duodiff_amd.engine import Model
    B = 4
    em = uvit(TINY, 41, "bf16", B)[0].engine_model(B)
    ec = uvit(TINY_COND, 42, "bf16", B)[0].engine_model(B)
    ctx, lib = em.ctx, em.ctx.lib
    ee = Model(ctx, ModelParams.from_dict(TINY), B)
    ee.enable_early_exit("mlp_probe_per_layer")
    x0, _ = _images(B, ModelParams.from_dict(TINY), 43)
    y = labels(B, 10, 44)
    stream = side_stream()
    n = 3
    f = (C.c_float * n)(900.0, 600.0, 300.0)
    one = (C.c_float * n)(1.0, 1.0, 1.0)
    seeds3 = ctx._seeds_tensor([1, 2, 3])

    def args(model=em, **over):
        a = L.dd_scan_args()
        a.model, a.x0_dev, a.y_dev, a.B, a.n_steps = model.handle, x0.data_ptr(), None, B, n
        a.t, a.ka, a.kb, a.tz, a.t0, a.tx = f, one, one, one, one, one
        a.seed, a.counter_base, a.noise_mode, a.use_graph = 1, 0, L.DD_NOISE_PHILOX, 1
        for k, v in over.items():
            setattr(a, k, v)
        return a

    cases = [(dict(x0_dev=None), "null"), (dict(err_dev=None), "null"), (dict(t=None), "null"), (dict(ka=None), "null"), (dict(tx=None), "null"),
             (dict(n_steps=0), "n_steps"), (dict(n_steps=(1 << 20) + 1), "n_steps"), (dict(counter_base=-1), "counter_base"),
             (dict(noise_mode=L.DD_NOISE_NONE), "noise_mode"), (dict(noise_mode=L.DD_NOISE_BUFFER), "noise_mode"),
             (dict(model=ee), "early_exit"), (dict(model=ec), "without labels"), (dict(y_dev=y.data_ptr()), "with labels"),
             (dict(B=B + 1), "max_batch"), (dict(B=0), "max_batch"), (dict(seeds=True), "seeds")]
    n0 = lib.dd_dev_graph_captures(ctx.handle)
    for over, msg in cases:
        err = torch.full((n, B + 1), -7.0, device="cuda")
        over = dict(over)
        seeded = over.pop("seeds", False)
        model = over.pop("model", em)
        a = args(model, **{"err_dev": err.data_ptr(), **over})
        if seeded:
            ctx.check(lib.dd_set_image_seeds(ctx.handle, C.c_void_p(seeds3.data_ptr()), 3))
        with torch.cuda.stream(stream):
            rc = lib.dd_scan_error(ctx.handle, C.byref(a), C.c_void_p(stream.cuda_stream))
        stream.synchronize()
        if seeded:
            ctx.check(lib.dd_set_image_seeds(ctx.handle, None, 0))
        assert rc == L.DD_ERR_INVALID, f"{msg}: status {rc}"
        assert msg in lib.dd_last_error(ctx.handle).decode(), (msg, lib.dd_last_error(ctx.handle).decode())
        assert bool((err == -7.0).all()), f"{msg}: something was enqueued"
    assert lib.dd_scan_error(ctx.handle, None, None) == L.DD_ERR_INVALID and lib.dd_scan_error(None, C.byref(args()), None) == L.DD_ERR_INVALID
    assert lib.dd_dev_graph_captures(ctx.handle) == n0
    err = torch.full((n, B), -7.0, device="cuda")                        # the same arguments with nothing overridden are accepted
    with torch.cuda.stream(stream):
        assert lib.dd_scan_error(ctx.handle, C.byref(args(err_dev=err.data_ptr())), C.c_void_p(stream.cuda_stream)) == L.DD_OK
    stream.synchronize()
    assert bool(torch.isfinite(err).all()) and bool((err >= 0).all())


def test_cli_end_to_end(tmp_path):
    """synthetic weights and 6 random images: a pair, a single model, and a pair of one model with itself (gap exactly 0, t_switch 1000)"""
    import yaml
    from duodiff_amd import switch_scan
    for name, depth, seed in (("s", 1, 51), ("f", 3, 52)):
        cfg = dict(TINY, depth=depth)
        (tmp_path / f"{name}.yaml").write_text(yaml.safe_dump({"model_params": cfg}))
        torch.save(dict(synthetic_state_dict(ModelParams.from_dict(cfg), seed)), tmp_path / f"{name}.pth")
    np.save(tmp_path / "x.npy", np.random.default_rng(53).uniform(-1, 1, (6, 3, 8, 8)).astype(F32))

    def run(out, *extra):
        switch_scan.main(["--config_path", str(tmp_path / "s.yaml"), "--checkpoint_path", str(tmp_path / "s.pth"), "--parametrization", "predict_noise",
                          "--images", str(tmp_path / "x.npy"), "--output_folder", str(tmp_path / out), "--timesteps", "999", "500", "1", "0", "--seed", "5",
                          *extra])
        return json.loads((tmp_path / out / "scan.json").read_text()), np.load(tmp_path / out / "scan.npz")

    late = ["--config_path_late", str(tmp_path / "f.yaml"), "--checkpoint_path_late", str(tmp_path / "f.pth")]
    js, npz = run("pair", *late, "--repeats", "2")
    assert js["timesteps"] == GRID and js["images"] == 6 and js["repeats"] == 2 and set(js["models"]) == {"first", "late"}
    assert npz["err_first"].shape == npz["err_late"].shape == (2, 4, 6) and npz["image_seeds"].tolist() == [5, 6, 7, 8, 9, 10]
    assert np.isfinite(npz["err_first"]).all() and (npz["err_late"] > 0).all()
    assert not np.array_equal(npz["err_first"][0], npz["err_first"][1])                   # the repeats draw fresh noise
    assert not np.array_equal(npz["err_first"], npz["err_late"])
    per = [npz[k].astype(np.float64).mean(0) for k in ("err_first", "err_late")]
    assert js["t_switch"] == switch_scan.suggest_t_switch(GRID, per[0], per[1], 0.02, 2.0)
    assert np.allclose(js["gap"], (per[0] - per[1]).mean(1) / per[1].mean(1), rtol=1e-9)
    js1, npz1 = run("single")
    assert set(js1["models"]) == {"first"} and "t_switch" not in js1 and set(npz1.files) == {"timesteps", "image_seeds", "err_first"}
    assert np.array_equal(npz1["err_first"][0], npz["err_first"][0])                      # the same (x0, z, t) as in the pair
    js2, npz2 = run("same", "--config_path_late", str(tmp_path / "s.yaml"), "--checkpoint_path_late", str(tmp_path / "s.pth"), "--no_graph")
    assert np.array_equal(npz2["err_first"], npz2["err_late"]) and np.array_equal(npz2["err_first"][0], npz["err_first"][0])
    assert js2["gap"] == [0.0] * 4 and js2["sem"] == [0.0] * 4 and js2["t_switch"] == 1000 and js2["advice"] == "--t_switch 1000"
