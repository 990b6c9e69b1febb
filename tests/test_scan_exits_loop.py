"""The early-exit scan as a device-resident loop (dd_scan_error_early_exit through engine.scan_exits_loop), on the GPU: bit-equal in all three
tables to its manual composition dev diffuse -> forward_early_exit(t) -> dev exits error for every probe type (the per-timestep probe
layouts pin that the step state holds the TIMESTEP), graph replay against eager launches, two chains against one, image seeds, graph reuse
and staleness, the loops around it unchanged, poisoned workspaces, one full-width case against dd_scan_error of the plain backbone, the numpy
oracle fed the kernel's own x_t (fp32 engine), the sampler's selection against simulate_exits, every rejection, the command line."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import kernel_support as ks
from conftest import TINY
from duodiff_amd import _lib as L
from duodiff_amd import step_plan, threshold_scan
from duodiff_amd.config import ModelParams
from duodiff_amd.weights import synthetic_ee_state_dict
from kernel_support import F32
from loop_support import dev_flags, ee_uvit, images, labels, side_stream, uvit
from scan_support import _images, diffuse, exits_error
from scan_support import _scan as _scan_loop
from test_early_exit import CASES

pytestmark = pytest.mark.gpu

GRID = [999, 500, 1, 0]
BY_TAG = {tag: (cfg, ctype) for tag, cfg, ctype in CASES}
NAMES = ("mse", "target", "pred")
CELEBA_EE = dict(img_size=64, patch_size=4, in_chans=3, embed_dim=512, depth=13, num_heads=8, mlp_ratio=4, qkv_bias=False, mlp_time_embed=False,
                 num_classes=-1, normalize_timesteps=True)


def _scan(*args, **kw):
    from duodiff_amd.engine import scan_exits_loop
    return _scan_loop(scan_exits_loop, *args, **kw)


def _scan_plain(*args, **kw):
    from duodiff_amd.engine import scan_error_loop
    return _scan_loop(scan_error_loop, *args, **kw)


def _same(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def _manual(em, x0, rows, y, seed, counter_base=0, seeds=None):
    """dev diffuse -> forward_early_exit at the timestep -> dev exits error, step by step: (mse, target, pred) and the x_t per step"""
    x0h = x0.cpu().numpy()
    B = x0h.shape[0]
    tabs, xts = ([], [], []), []
    for k in range(len(rows["t"])):
        kw = dict(ka=rows["ka"][k], kb=rows["kb"][k], ctr=counter_base + k, seed=seed, seeds=seeds)
        xt = diffuse(x0h, 0, B, **kw)[0]
        eps, cls, outs = em.forward_early_exit(torch.from_numpy(xt).cuda(), float(rows["t"][k]), y)
        planes = np.concatenate([outs.cpu().numpy(), eps.cpu().numpy()[None]])
        r = exits_error(x0h, planes, cls.cpu().numpy(), 0, B, (rows["tz"][k], rows["t0"][k], rows["tx"][k]), k=0, t=int(rows["t"][k]), nxt=0, **kw)
        for dst, name in zip(tabs, ("mse", "tgtu", "pred")):
            dst.append(r[name])
        xts.append(xt)
    return tuple(np.stack(t) for t in tabs), np.stack(xts)


@pytest.mark.parametrize("tag", sorted(BY_TAG))
def test_loop_equals_manual_composition_and_graph_equals_eager(tag):
    cfg, ctype = BY_TAG[tag]
    B = 5
    m, mp = ee_uvit(cfg, 11, ctype, "bf16", B)
    em = m.engine_model(B)
    x0, y = _images(B, mp, 12)
    for par in ("predict_noise", "predict_original") if tag == "layer" else ("predict_noise",):
        rows = step_plan.scan_rows(GRID, par)
        want = _manual(em, x0, rows, y, seed=77, counter_base=8)[0]
        eager = _scan(em, x0, rows, y, seed=77, counter_base=8, use_graph=False)
        graph = _scan(em, x0, rows, y, seed=77, counter_base=8, use_graph=True)
        assert all(np.isfinite(w).all() for w in want) and (want[0] > 0).all() and (want[1] > 0).all() and (want[1] < 1).all()
        for name, e, w in zip(NAMES, eager, want):
            assert np.array_equal(e.view(np.uint32), w.view(np.uint32)), f"{tag} {par}: {name} of the eager loop differs from diffuse -> forward_early_exit -> exits error"
        assert _same(graph, eager), f"{tag} {par}: graph replay differs from the eager launches"
    if "timestep" in ctype:       # the probes of two timesteps differ: a loop that took the row index for the timestep would show here
        assert not np.array_equal(want[2][0], want[2][1])
    assert not _same(_scan(em, x0, rows, y, seed=77, counter_base=9)[:2], graph[:2])        # other counters: other z
    # the grid in another order: the same rows, permuted (the table is indexed by timestep, the output by the step)
    perm = [2, 0, 3, 1]
    rows_p = {k: v[perm] for k, v in rows.items()}
    got = _scan(em, x0, rows_p, y, seed=77, counter_base=8, use_graph=False)
    assert _same(got, _manual(em, x0, rows_p, y, seed=77, counter_base=8)[0])


def test_image_seeds_an_image_does_not_depend_on_its_batch():
    B = 6
    cfg, ctype = BY_TAG["timestep"]
    m, mp = ee_uvit(cfg, 13, ctype, "bf16", B)
    em = m.engine_model(B)
    x0, _ = _images(B, mp, 14)
    rows = step_plan.scan_rows(GRID, "predict_noise")
    seeds = [1000 + 7 * i for i in range(B)]
    with em.ctx.image_seeds(seeds):
        whole = _scan(em, x0, rows, seed=1)
        again = _scan(em, x0, rows, seed=2)                              # the call's own seed is unused
    want = _manual(em, x0, rows, None, seed=0, seeds=np.array(seeds, np.uint64))[0]
    assert _same(whole, want) and _same(again, whole)
    with em.ctx.image_seeds(seeds[2:5]):
        part = _scan(em, x0[2:5].contiguous(), rows)
    assert _same(part, tuple(w[:, :, 2:5] for w in whole)), "an image's numbers depend on the batch it ran in"
    assert not _same(_scan(em, x0, rows, seed=1)[:2], whole[:2])       # without the seeds: the plain draw


def test_two_chains_equal_one():
    B = 4
    cfg, ctype = BY_TAG["layer_timestep_cond"]
    m, mp = ee_uvit(cfg, 15, ctype, "bf16", B)
    em = m.engine_model(B)
    ctx = em.ctx
    x0, y = _images(B, mp, 16)
    rows = step_plan.scan_rows(GRID, "predict_original")
    outs = {}
    for name, flags in (("chained", L.DD_DEV_FORCE_CHAINS), ("single", L.DD_DEV_NO_CHAINS)):
        with dev_flags(ctx, flags):
            outs[name] = (_scan(em, x0, rows, y, seed=5), ctx.lib.dd_dev_last_sample_chains(ctx.handle))
    assert outs["chained"][1] == 2 and outs["single"][1] == 1
    assert all(np.isfinite(o).all() for o in outs["single"][0])
    assert _same(outs["chained"][0], outs["single"][0]), "the two half-batch chains differ from the single chain"
    # chain 0 of two (2 images from image 0, rows of 4) is not the whole batch's captured step of 2 images
    with dev_flags(ctx, L.DD_DEV_NO_CHAINS):
        half = _scan(em, x0[:2].contiguous(), rows, y[:2].contiguous(), seed=5)
    with dev_flags(ctx, L.DD_DEV_FORCE_CHAINS):
        both = _scan(em, x0, rows, y, seed=5)
    with dev_flags(ctx, L.DD_DEV_NO_CHAINS):
        assert _same(_scan(em, x0[:2].contiguous(), rows, y[:2].contiguous(), seed=5), half)
    assert _same(both, outs["single"][0]) and _same(half, tuple(b[:, :, :2] for b in both))


def test_graph_reuse_and_no_stale_graph():
    """other tensors of the same shape replay the captured step; another grid, target or counter base is honoured by the replay"""
    B = 3
    cfg, ctype = BY_TAG["timestep"]
    m, mp = ee_uvit(cfg, 17, ctype, "bf16", B)
    em = m.engine_model(B)
    ctx = em.ctx
    rows = step_plan.scan_rows(GRID, "predict_noise")
    xa, _ = _images(B, mp, 18)
    xb, _ = _images(B, mp, 19)
    stream = side_stream()
    first = _scan(em, xa, rows, seed=3, stream=stream)
    n0 = ctx.lib.dd_dev_graph_captures(ctx.handle)
    second = _scan(em, xb, rows, seed=3, stream=stream)
    assert ctx.lib.dd_dev_graph_captures(ctx.handle) == n0, "a second call with other tensors of the same shape captured again"
    assert _same(second, _scan(em, xb, rows, seed=3, use_graph=False)) and not _same(second, first)
    for other, base in ((step_plan.scan_rows([900, 600, 300, 7], "predict_noise"), 0), (step_plan.scan_rows(GRID, "predict_original"), 0),
                        (rows, 4), (step_plan.scan_rows(GRID[::-1], "predict_noise"), 0)):
        got = _scan(em, xa, other, seed=3, counter_base=base, stream=stream)
        assert _same(got, _scan(em, xa, other, seed=3, counter_base=base, use_graph=False)), "replayed the step of another grid, target or base"
        assert not _same(got[:2], first[:2])
    assert ctx.lib.dd_dev_graph_captures(ctx.handle) == n0               # rows and base live in a device table: none of these captured again
    assert _same(_scan(em, xa, rows, seed=3, stream=stream), first)
    shorter = step_plan.scan_rows(GRID[:3], "predict_noise")             # another number of rows: other tables, captured again, and right
    assert _same(_scan(em, xa, shorter, seed=3, stream=stream), tuple(f[:3] for f in first))


def test_loops_around_a_scan_are_unchanged():
    """dd_sample_early_exit of the same model and dd_scan_error of a plain model (which shares the context's row table and scratch) before and
    after an early-exit scan: bit for bit"""
    from duodiff_amd.engine import sample_early_exit_loop
    B = 4
    cfg, ctype = BY_TAG["layer"]
    m, mp = ee_uvit(cfg, 21, ctype, "bf16", B)
    em = m.engine_model(B)
    plain = uvit(TINY, 21, "bf16", B)[0].engine_model(B)
    ctx = em.ctx
    xT = images(B, 3, 8, 22)
    x0, _ = _images(B, mp, 23)
    rows = step_plan.scan_rows(GRID, "predict_noise")
    stream = side_stream()

    def sample():
        x = xT.clone()
        err = torch.zeros(1000, mp.depth, device="cuda")
        idx = torch.zeros(1000, B, device="cuda", dtype=torch.int32)
        with torch.cuda.stream(stream):
            sample_early_exit_loop(ctx, em, x, 0.4, t_start=999, t_end=995, seed=9, err=err, idx=idx, stream=stream)
        stream.synchronize()
        return x, err, idx

    before = sample(), _scan_plain(plain, x0, rows, seed=9, stream=stream)
    scanned = _scan(em, x0, rows, seed=9, stream=stream)
    after = sample(), _scan_plain(plain, x0, rows, seed=9, stream=stream)
    assert all(np.isfinite(s).all() for s in scanned) and torch.isfinite(before[0][0]).all()
    assert all(torch.equal(a, b) for a, b in zip(before[0], after[0])), "a scan changed the early-exit sampling loop that follows it"
    assert np.array_equal(before[1], after[1]), "a scan changed the plain scan that follows it"
    assert _same(_scan(em, x0, rows, seed=9, stream=stream), scanned)
    # the backbone's exit is the plain model's error on the same weights, bit for bit
    assert np.array_equal(scanned[0][:, mp.depth], before[1])


def test_scan_reads_no_stale_workspace_bytes():
    B = 4
    cfg, ctype = BY_TAG["attention"]
    x0, _ = _images(B, ModelParams.from_dict(cfg), 25)
    rows = step_plan.scan_rows(GRID[:3], "predict_noise")
    outs = []
    for poison in (False, True):
        em = ee_uvit(cfg, 26, ctype, "bf16", B)[0].engine_model(B)
        ctx, stream = em.ctx, side_stream()
        with dev_flags(ctx, L.DD_DEV_FORCE_CHAINS):
            if poison:
                with torch.cuda.stream(stream):
                    ctx.check(ctx.lib.dd_dev_poison_workspaces(ctx.handle, em.handle, stream.cuda_stream))
            outs.append(_scan(em, x0, rows, seed=4, stream=stream))
            assert ctx.lib.dd_dev_last_sample_chains(ctx.handle) == 2
        del em
    assert all(np.isfinite(o).all() for o in outs[0]) and _same(outs[0], outs[1]), "the scan differs after the workspaces were poisoned"


def test_full_width_celeba_shape():
    """deediff_celeba's shape (D = 512, depth 13), synthetic weights, B = 2, bf16: the loop is its manual composition, and the backbone's
    exit is dd_scan_error of the plain U-ViT with the same backbone weights, bit for bit"""
    B, grid = 2, [999, 0]
    m, mp = ee_uvit(CELEBA_EE, 61, "mlp_probe_per_layer", "bf16", B)
    em = m.engine_model(B)
    x0, _ = _images(B, mp, 62)
    rows = step_plan.scan_rows(grid, "predict_noise")
    got = _scan(em, x0, rows, seed=6)
    assert got[0].shape == (2, 14, B) and got[2].shape == (2, 13, B) and all(np.isfinite(g).all() for g in got)
    assert _same(got, _manual(em, x0, rows, None, seed=6)[0])
    assert _same(got, _scan(em, x0, rows, seed=6, use_graph=False))
    plain = uvit(CELEBA_EE, 61, "bf16", B)[0].engine_model(B)
    assert np.array_equal(got[0][:, 13], _scan_plain(plain, x0, rows, seed=6))


@pytest.mark.parametrize("tag", sorted(BY_TAG))
def test_against_the_oracle_fp32(tag):
    """The oracle (float64 numpy) is fed the kernel's own x_t; both losses are taken in float64 from the kernel's own z.  fp32 engine: every
    output is within delta = 1e-4 of the oracle's elementwise (the forward bound the suite already uses), so mse is within 2 delta sqrt(want)
    + delta^2 (Cauchy-Schwarz) and the mean of the 1-Lipschitz tanh|.| within delta; pred within the 1e-5 / 2e-5 the suite uses for cls."""
    import oracle
    from scan_support import draw
    cfg, ctype = BY_TAG[tag]
    B = 3
    mp = ModelParams.from_dict(cfg)
    sd = synthetic_ee_state_dict(mp, 31, ctype)
    orc = oracle.EarlyExitOracle(mp.as_dict(), {k: v.numpy() for k, v in sd.items()}, ctype)
    x0, y = _images(B, mp, 32)
    x0h, yh = x0.cpu().numpy(), None if y is None else y.cpu().numpy()
    rows = step_plan.scan_rows(GRID, "predict_noise")
    want_m, want_u, want_p = [], [], []
    for k, t in enumerate(GRID):
        z = draw(B, mp.in_chans, mp.img_size, 0, B, ctr=k, seed=55).astype(np.float64)
        xt = diffuse(x0h, 0, B, ka=rows["ka"][k], kb=rows["kb"][k], ctr=k, seed=55)[0]
        eps, cls, outs = orc(xt, np.full((B,), t, np.float32), yh)
        d = np.stack(list(outs) + [eps]).astype(np.float64) - z[None]          # predict_noise: the target is z
        want_m.append((d * d).mean((2, 3, 4)))
        want_u.append(np.tanh(np.abs(d)).mean((2, 3, 4)))
        want_p.append(np.stack(cls))
    want_m, want_u, want_p = np.stack(want_m), np.stack(want_u), np.stack(want_p)
    em = ee_uvit(cfg, 31, ctype, "fp32", B)[0].engine_model(B)
    mse, target, pred = _scan(em, x0, rows, y, seed=55)
    delta = 1e-4
    r_m = ks.gate(mse, want_m, 2 * delta * np.sqrt(want_m) + delta ** 2, f"{tag}: mse against the oracle")
    r_u = ks.gate(target, want_u, delta, f"{tag}: target against the oracle")
    r_p = ks.gate(pred, want_p, 2e-5 if ctype == "attention_probe" else 1e-5, f"{tag}: pred against the oracle")
    print(f"{tag}: observed / bound  mse {r_m:.3f}  target {r_u:.3f}  pred {r_p:.3f}")


def test_the_samplers_selection_is_simulate_exits():
    B = 6
    cfg, ctype = BY_TAG["layer"]
    m, mp = ee_uvit(cfg, 35, ctype, "bf16", B)
    em = m.engine_model(B)
    x0, _ = _images(B, mp, 36)
    rows = step_plan.scan_rows(GRID, "predict_noise")
    mse, target, pred = _scan(em, x0, rows, seed=8)
    flat = np.sort(pred.ravel())
    thresholds = [float(flat[0]), float(flat[len(flat) // 3]), float(flat[len(flat) // 2]), float(flat[-1]), 0.0, float(np.nextafter(flat[len(flat) // 2], F32(0)))]
    outs, eps = torch.zeros(mp.depth, B, 3, 8, 8, device="cuda"), torch.zeros(B, 3, 8, 8, device="cuda")
    for thr in thresholds:
        idx = threshold_scan.simulate_exits(pred, thr)
        for k in range(len(GRID)):
            got = em.ctx.early_exit_select(outs, eps, torch.from_numpy(pred[k]).cuda(), thr)[1].cpu().numpy()
            assert np.array_equal(got, idx[k]), (thr, k)
    assert len({int(threshold_scan.simulate_exits(pred, t).sum()) for t in thresholds}) > 2       # the thresholds tell exits apart


def test_invalid_calls_are_rejected_before_anything_is_enqueued():
    B = 4
    cfg, ctype = BY_TAG["layer"]
    em = ee_uvit(cfg, 41, ctype, "bf16", B)[0].engine_model(B)
    ec = ee_uvit(BY_TAG["attention_cond"][0], 42, "attention_probe", "bf16", B)[0].engine_model(B)
    plain = uvit(TINY, 43, "bf16", B)[0].engine_model(B)
    ctx, lib = em.ctx, em.ctx.lib
    depth = 3
    x0, _ = _images(B, ModelParams.from_dict(TINY), 43)
    y = labels(B, 10, 44)
    stream = side_stream()
    n = 3
    f = (C.c_float * n)(900.0, 600.0, 300.0)
    one = (C.c_float * n)(1.0, 1.0, 1.0)
    seeds3 = ctx._seeds_tensor([1, 2, 3])
    keep = []

    def args(model=em, **over):
        a = L.dd_scan_exits_args()
        a.model, a.x0_dev, a.y_dev, a.B, a.n_steps = model.handle, x0.data_ptr(), None, B, n
        a.t, a.ka, a.kb, a.tz, a.t0, a.tx = f, one, one, one, one, one
        a.seed, a.counter_base, a.noise_mode, a.use_graph = 1, 0, L.DD_NOISE_PHILOX, 1
        for k, v in over.items():
            if k == "t" and v is not None:
                v = (C.c_float * n)(*v)
                keep.append(v)
            setattr(a, k, v)
        return a

    cases = [(dict(x0_dev=None), "null"), (dict(mse_dev=None), "null"), (dict(target_dev=None), "null"), (dict(pred_dev=None), "null"),
             (dict(t=None), "null"), (dict(ka=None), "null"), (dict(tx=None), "null"),
             (dict(n_steps=0), "n_steps"), (dict(n_steps=(1 << 20) + 1), "n_steps"), (dict(counter_base=-1), "counter_base"),
             (dict(counter_base=(1 << 20) + 1), "counter_base"),
             (dict(noise_mode=L.DD_NOISE_NONE), "noise_mode"), (dict(noise_mode=L.DD_NOISE_BUFFER), "noise_mode"),
             (dict(t=(900.0, 600.5, 300.0)), "not an integer"), (dict(t=(900.0, 1000.0, 300.0)), "not an integer"),
             (dict(t=(900.0, -1.0, 300.0)), "not an integer"), (dict(t=(900.0, float("nan"), 300.0)), "not an integer"),
             (dict(t=(900.0, 300.0, 900.0)), "occurs twice"),
             (dict(model=ec), "without labels"), (dict(y_dev=y.data_ptr()), "with labels"),
             (dict(B=B + 1), "max_batch"), (dict(B=0), "max_batch"), (dict(seeds=True), "seeds")]
    n0 = lib.dd_dev_graph_captures(ctx.handle)

    def call(a):
        with torch.cuda.stream(stream):
            rc = lib.dd_scan_error_early_exit(ctx.handle, C.byref(a), C.c_void_p(stream.cuda_stream))
        stream.synchronize()
        return rc

    def outputs():
        return [torch.full((n, depth + 1, B + 1), -7.0, device="cuda") for _ in range(3)]

    for over, msg in cases:
        o = outputs()
        over = dict(over)
        seeded = over.pop("seeds", False)
        model = over.pop("model", em)
        a = args(model, **{"mse_dev": o[0].data_ptr(), "target_dev": o[1].data_ptr(), "pred_dev": o[2].data_ptr(), **over})
        if seeded:
            ctx.check(lib.dd_set_image_seeds(ctx.handle, C.c_void_p(seeds3.data_ptr()), 3))
        rc = call(a)
        if seeded:
            ctx.check(lib.dd_set_image_seeds(ctx.handle, None, 0))
        assert rc == L.DD_ERR_INVALID, f"{msg}: status {rc}"
        assert msg in lib.dd_last_error(ctx.handle).decode(), (msg, lib.dd_last_error(ctx.handle).decode())
        assert all(bool((t == -7.0).all()) for t in o), f"{msg}: something was enqueued"
    # a plain model: DD_ERR_STATE with dd_sample_early_exit's message
    o = outputs()
    assert call(args(plain, mse_dev=o[0].data_ptr(), target_dev=o[1].data_ptr(), pred_dev=o[2].data_ptr())) == L.DD_ERR_STATE
    assert "model was not created with dd_model_enable_early_exit" in lib.dd_last_error(ctx.handle).decode()
    assert all(bool((t == -7.0).all()) for t in o)
    # unsupported shapes: DD_ERR_UNSUPPORTED.  Model creation refuses in_chans outside 1..4 of the scan's range and images of more than 2^24
    # elements never fit a test, so those two branches are out of reach here; depth + 1 > 32 is not: dd_model_create takes any odd depth
    deep = ee_uvit(dict(TINY, depth=33), 45, "mlp_probe_per_layer", "bf16", B)[0].engine_model(B)
    o = [torch.full((n, 34, B), -7.0, device="cuda") for _ in range(3)]
    assert call(args(deep, mse_dev=o[0].data_ptr(), target_dev=o[1].data_ptr(), pred_dev=o[2].data_ptr())) == L.DD_ERR_UNSUPPORTED
    assert "at most 32 exits" in lib.dd_last_error(ctx.handle).decode()
    assert all(bool((t == -7.0).all()) for t in o), "depth 33: something was enqueued"
    shallower = ee_uvit(dict(TINY, depth=31), 46, "mlp_probe_per_layer", "bf16", B)[0].engine_model(B)      # 32 exits: the largest accepted
    o = [torch.full((n, 32, B), -7.0, device="cuda"), torch.full((n, 32, B), -7.0, device="cuda"), torch.full((n, 31, B), -7.0, device="cuda")]
    n1 = lib.dd_dev_graph_captures(ctx.handle)
    assert n1 == n0, "a rejected call captured a graph"
    assert call(args(shallower, mse_dev=o[0].data_ptr(), target_dev=o[1].data_ptr(), pred_dev=o[2].data_ptr())) == L.DD_OK
    assert all(bool(torch.isfinite(t).all()) for t in o) and lib.dd_dev_graph_captures(ctx.handle) == n1 + 1
    n0 += 1
    assert lib.dd_scan_error_early_exit(ctx.handle, None, None) == L.DD_ERR_INVALID
    assert lib.dd_scan_error_early_exit(None, C.byref(args()), None) == L.DD_ERR_INVALID
    assert lib.dd_dev_graph_captures(ctx.handle) == n0
    o = [torch.full((n, depth + 1, B), -7.0, device="cuda"), torch.full((n, depth + 1, B), -7.0, device="cuda"), torch.full((n, depth, B), -7.0, device="cuda")]
    assert call(args(mse_dev=o[0].data_ptr(), target_dev=o[1].data_ptr(), pred_dev=o[2].data_ptr())) == L.DD_OK      # nothing overridden: accepted
    assert all(bool(torch.isfinite(t).all()) for t in o) and bool((o[0] >= 0).all()) and bool((o[1] >= 0).all())


def test_cli_end_to_end(tmp_path):
    """synthetic weights and 6 random images: the files' shapes, fresh noise per repeat, exits.json against the numpy functions on the saved
    arrays, and a threshold list of [0] on a model whose predictions are all positive (mean-of-sigmoid probes): gap exactly 0, every block run"""
    import yaml
    cfg = dict(TINY, classifier_type="mlp_probe_per_timestep")
    mp = ModelParams.from_dict(cfg)
    (tmp_path / "ee.yaml").write_text(yaml.safe_dump({"model_params": cfg}))
    torch.save(dict(synthetic_ee_state_dict(mp, 51, "mlp_probe_per_timestep")), tmp_path / "ee.pth")
    np.save(tmp_path / "x.npy", np.random.default_rng(53).uniform(-1, 1, (6, 3, 8, 8)).astype(F32))

    def run(out, *extra):
        threshold_scan.main(["--config_path", str(tmp_path / "ee.yaml"), "--checkpoint_path", str(tmp_path / "ee.pth"), "--parametrization", "predict_noise",
                             "--images", str(tmp_path / "x.npy"), "--output_folder", str(tmp_path / out), "--timesteps", "999", "500", "1", "0",
                             "--seed", "5", "--batch_size", "4", *extra])
        return json.loads((tmp_path / out / "exits.json").read_text()), np.load(tmp_path / out / "exits.npz")

    js, npz = run("a", "--repeats", "2", "--num_thresholds", "8", "--tolerance", "0.5")
    depth = mp.depth
    assert js["timesteps"] == GRID and js["images"] == 6 and js["repeats"] == 2 and js["depth"] == depth
    assert npz["mse"].shape == npz["target"].shape == (2, 4, depth + 1, 6) and npz["predicted"].shape == (2, 4, depth, 6)
    assert npz["timesteps"].tolist() == GRID and npz["image_seeds"].tolist() == [5, 6, 7, 8, 9, 10]
    assert all(np.isfinite(npz[k]).all() for k in ("mse", "target", "predicted")) and (npz["mse"] > 0).all()
    assert not np.array_equal(npz["mse"][0], npz["mse"][1])                              # the repeats draw fresh noise
    assert not np.array_equal(npz["predicted"][0], npz["predicted"][1])
    mse, pred = npz["mse"].astype(np.float64), npz["predicted"]
    assert np.allclose(js["mean_mse"], mse.mean(axis=(0, 3)), rtol=1e-12) and np.allclose(js["mean_predicted"], pred.astype(np.float64).mean(axis=(0, 3)), rtol=1e-12)
    cands = threshold_scan.candidate_thresholds(pred, num_thresholds=8)
    assert [row["threshold"] for row in js["candidates"]] == cands and 1 < len(cands) <= 8
    gaps, sems = [], []
    for row in js["candidates"]:
        idx = np.stack([threshold_scan.simulate_exits(pred[r], row["threshold"]) for r in range(2)])
        gap, sem, blocks = threshold_scan.threshold_statistics(mse, idx)
        assert np.allclose(row["gap"], gap, rtol=1e-12, atol=1e-15) and np.allclose(row["sem"], sem, rtol=1e-12, atol=1e-15)
        assert row["blocks_fraction"] == pytest.approx(blocks)
        gaps.append(gap); sems.append(sem)
    # ... and threshold_statistics itself against the definition, written out once for the repeats axis
    realised = np.stack([[[mse[r, k, idx[r, k, i], i] for i in range(6)] for k in range(4)] for r in range(2)]).mean(0)
    back = mse[:, :, depth, :].mean(0)
    assert np.allclose(gap, (realised - back).mean(1) / back.mean(1), rtol=1e-12, atol=1e-15)
    assert np.allclose(sem, (realised - back).std(1, ddof=1) / np.sqrt(6) / back.mean(1), rtol=1e-12, atol=1e-15) and blocks == pytest.approx(idx.mean() / depth)
    assert js["threshold"] == threshold_scan.suggest_threshold(cands, gaps, sems, 0.5, 2.0)
    cal = threshold_scan.calibration(pred.reshape(8, depth, 6), npz["target"].reshape(8, depth + 1, 6))
    assert np.allclose(js["calibration"]["rmse"], cal["rmse"]) and np.allclose(js["calibration"]["mean_target"], cal["mean_target"])
    js0, npz0 = run("zero", "--thresholds", "0", "--no_graph")
    assert (npz0["predicted"] > 0).all()
    assert np.array_equal(npz0["mse"][0], npz["mse"][0])                                 # the same (x0, z, t), eagerly
    row = js0["candidates"][0]
    assert row["gap"] == [0.0] * 4 and row["sem"] == [0.0] * 4 and row["blocks_fraction"] == 1.0
    assert js0["threshold"] == 0.0 and js0["advice"].startswith("--threshold 0")
    # per-image seeds: the batches of 4 + 2 images give what one batch of 6 gives
    js6, npz6 = run("six", "--thresholds", "0", "--batch_size", "6")
    assert np.array_equal(npz6["mse"], npz0["mse"]) and np.array_equal(npz6["predicted"], npz0["predicted"])
