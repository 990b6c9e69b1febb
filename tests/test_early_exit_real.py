"""Real early exit (dd_sample_early_exit_real): the early-exit loop with the exits taken.  An image that has left runs no further block;
the batch is compacted between blocks.  Acceptance: every image and every idx row equals the simulated loop's (dd_sample_early_exit) bit
for bit -- a row takes the same kernels in any slot of any batch -- and the run provably launches fewer block-rows."""
import ctypes as C

import numpy as np
import pytest
import torch

from duodiff_amd.config import ModelParams
from duodiff_amd.early_exit import real_exit_block_rows
from duodiff_amd.weights import synthetic_ee_state_dict, synthetic_state_dict

from conftest import GOLDEN, REPO, TINY
from loop_support import dev_flags

pytestmark = pytest.mark.gpu

PROBES = [("mlp_probe_per_layer", dict(TINY)), ("mlp_probe_per_timestep", dict(TINY)),
          ("mlp_probe_per_layer_per_timestep", dict(TINY, num_classes=10)), ("attention_probe", dict(TINY))]


def _engine(cfg, seed, ctype, precision, max_batch=None, hold=0):       # (as tests/test_early_exit.py builds its models)
    """hold > 0 (mlp_probe_per_layer): the probes of layers [0, hold) get a bias of +30 -- their prediction is 1 to the last bit, above any
    threshold in use, so no image leaves in front of layer `hold` and the exits fall on the layers behind it: the synthetic probes'
    own predictions drop so fast with depth that otherwise every image has left by the second layer."""
    from duodiff_amd.early_exit import EarlyExitUViT
    from duodiff_amd.uvit import UViT
    mp = ModelParams.from_dict(cfg)
    m = EarlyExitUViT(UViT(**mp.as_dict(), precision=precision, max_batch=max_batch), ctype)
    sd = synthetic_ee_state_dict(mp, seed, ctype)
    for l in range(hold):
        sd[f"matrix.{l}.classifier.0.bias"] = sd[f"matrix.{l}.classifier.0.bias"] + 30.0
    m.load_state_dict(sd)
    return m.eval().to("cuda"), mp


def _first_cls(m, mp, B, y=None, seed=1):
    S = mp.img_size
    x = torch.randn(B, mp.in_chans, S, S, generator=torch.Generator().manual_seed(seed))
    _, cls, _ = m.forward_device(x, torch.full((B,), 999.0), y)
    return cls.cpu()


def _run(m, mp, B, thr, noise, steps, y=None, image_seeds=None, compact_every=1, stats=None, seed=5):
    from duodiff_amd import eesampler
    S = mp.img_size
    samples, _, ind = eesampler.get_samples(m, B, seed, mp.in_chans, S, S, thr, mp.depth, y=y, noise=noise, num_steps=steps,
                                            image_seeds=image_seeds, compact_every=compact_every, stats=stats)
    return samples, ind[1000 - steps:]


def _moves_of_step(idx_row, depth, s):
    """numpy restatement of one step of one chain: (block-rows, moves) for the exit indices of the chain's images, by the kernel's rule"""
    slots = list(range(len(idx_row)))           # slot -> image
    rows = moves = 0
    for l in range(depth):
        if l % s == 0:
            alive = [idx_row[i] > l for i in slots]          # an image with exit index e has left once layer e's probe has run
            keep = sum(alive)
            holes = [d for d in range(keep) if not alive[d]]
            srcs = [q for q in range(keep, len(slots)) if alive[q]]
            assert len(holes) == len(srcs)
            for src, dst in zip(srcs, holes):
                slots[dst], slots[src] = slots[src], slots[dst]
            moves += len(holes)
            slots = slots[:keep]
        rows += len(slots)
    return rows, moves


def _expected(idx, depth, s, halves):
    """(block-rows, moves) of a whole run from its idx table [steps, B]; halves: the chains' column ranges"""
    rows = moves = 0
    for row in idx.numpy().astype(int):
        for lo, hi in halves:
            r, mv = _moves_of_step(list(row[lo:hi]), depth, s)
            rows, moves = rows + r, moves + mv
    return rows, moves


# ---------------------------------------------------------------- 1. bit identity
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("ctype,cfg", PROBES)
def test_real_exit_equals_the_simulated_loop_tiny(ctype, cfg, precision):
    """Case A: TINY, B = 3 and 6, every probe type, compact_every in {1, 2, depth + 1}, one chain and two, per-image seeds."""
    from duodiff_amd import _lib as L
    m, mp = _engine(cfg, 91, ctype, precision)
    depth = mp.depth
    for B, steps in ((6, 60), (3, 90)):
        y = torch.tensor([1, 7, 3, 0, 9, 4][:B]) if cfg.get("num_classes", -1) > 0 else None
        cls0 = _first_cls(m, mp, B, y)
        thr = float(cls0.median())          # inside the spread of the predicted errors: the run takes more than one exit
        ctx = m.engine_model(B).ctx
        with dev_flags(ctx, L.DD_DEV_NO_CHAINS):
            want = {n: _run(m, mp, B, thr, n, steps, y) for n in ("device_none", "device")}
            want["seeded"] = _run(m, mp, B, thr, "device", steps, y, image_seeds=list(range(40, 40 + B)))
        assert len(set(want["device_none"][1].flatten().tolist())) > 1, "the run should take more than one exit"
        assert not np.array_equal(want["device"][0], want["seeded"][0])
        for flags, chains in ((L.DD_DEV_NO_CHAINS, 1), (L.DD_DEV_FORCE_CHAINS, 2 if B % 2 == 0 else 1)):
            with dev_flags(ctx, flags):
                for s in (1, 2, depth + 1):
                    for name, noise, seeds in (("device_none", "device_real_none", None), ("device", "device_real", None),
                                               ("seeded", "device_real", list(range(40, 40 + B)))):
                        got, g_ind = _run(m, mp, B, thr, noise, steps, y, image_seeds=seeds, compact_every=s)
                        assert ctx.lib.dd_dev_last_sample_chains(ctx.handle) == chains
                        where = f"{ctype} {precision} B {B} chains {chains} compact_every {s} {name}"
                        assert torch.equal(g_ind, want[name][1]), f"{where}: exit indices differ"
                        assert np.array_equal(got, want[name][0]), f"{where}: images differ"


def _pick_threshold(m, mp, B, steps, seed=1, hold=0):
    """A threshold inside the spread of the predicted errors, chosen on the SIMULATED loop alone: the first of a few quantiles of a first
    forward's predictions (the median of the first layer that lets images go first: about half of them leave there, the others further
    down) with which that loop takes more than one exit, none in front of layer `hold`.  Returns it with that loop's result."""
    cls0 = _first_cls(m, mp, B, seed=seed)[hold:]
    for thr in (float(cls0[0].median()), float(cls0.median()), float(cls0[len(cls0) // 2].median()), float(cls0.quantile(0.25))):
        want, w_ind = _run(m, mp, B, thr, "device", steps)
        if len(set(w_ind.flatten().tolist())) > 1 and float(w_ind.min()) >= hold:
            return thr, want, w_ind
    raise AssertionError("none of the candidate thresholds makes the simulated loop take more than one exit")


def _check_case(m, mp, B, steps, picked, sweeps=((1, 0), (2, 0))):
    ctx = m.engine_model(B).ctx
    thr, want, w_ind = picked
    assert np.isfinite(want).all()
    for s, flags in sweeps:
        with dev_flags(ctx, flags):
            st = {}
            got, g_ind = _run(m, mp, B, thr, "device_real", steps, compact_every=s, stats=st)
        print(f"B {B} compact_every {s} flags {flags}: block-rows {st['block_rows']} of {st['block_rows_full']}, moves {st['moves']}")
        assert torch.equal(g_ind, w_ind), f"compact_every {s}: exit indices differ"
        assert np.array_equal(got, want), f"compact_every {s}: images differ"
        assert st["block_rows"] == real_exit_block_rows(w_ind, mp.depth, s) < st["block_rows_full"]
    return ctx


CASE_B = dict(img_size=32, patch_size=4, in_chans=3, embed_dim=256, depth=13, num_heads=4, mlp_ratio=4, qkv_bias=False,
              mlp_time_embed=False, num_classes=-1, normalize_timesteps=True)


@pytest.fixture(scope="module")
def case_b():
    """(model, params, (threshold, the simulated loop's images, its idx rows)) of Case B with the exits behind the mid block"""
    m, mp = _engine(CASE_B, 79, "mlp_probe_per_layer", "bf16", max_batch=8, hold=8)
    return m, mp, _pick_threshold(m, mp, 7, 3, hold=8)


@pytest.mark.parametrize("hold", [0, 3, 8])
def test_real_exit_odd_batch_non_batched_heads(case_b, hold):
    """Case B: embed_dim 256, depth 13, 65 tokens, max_batch 8, B = 7: an odd batch on the heads' non-batched path; an image's slab is no
    multiple of a 16-row tile, so slabs straddle row tiles.  The exits fall on the first layers, on the in-blocks from layer 3 on, and on
    the out-blocks from layer 8 on (whose skip_linear has run in the block tail in front)."""
    m, mp, picked = case_b if hold == 8 else (lambda m, mp: (m, mp, _pick_threshold(m, mp, 7, 3, hold=hold)))(
        *_engine(CASE_B, 79, "mlp_probe_per_layer", "bf16", max_batch=8, hold=hold))
    _check_case(m, mp, 7, 3, picked, sweeps=((1, 0), (2, 0), (5, 0)))


@pytest.mark.parametrize("hold", [0, 3, 8])
def test_real_exit_celeba_size_chained(hold):
    """Case C: the CelebA early-exit model, B = 32, bf16: the fused block tail, the fragment-order hand-offs, the fused skip_linear with the
    y tap, batched heads -- as two half-batch chains (the default policy at B = 32) and as one.  Exits on the first layers, from in-block 3
    on (long-skip copies and their fragment copies are live and move) and from out-block 8 on."""
    from duodiff_amd import _lib as L
    from duodiff_amd.config import load_config
    mpd = dict(load_config(REPO / "configs" / "deediff_celeba.yaml")["model_params"])
    ctype = mpd.pop("classifier_type")
    m, mp = _engine(mpd, 78, ctype, "bf16", max_batch=32, hold=hold)
    ctx = _check_case(m, mp, 32, 3, _pick_threshold(m, mp, 32, 3, seed=2, hold=hold), sweeps=((1, 0), (2, 0), (1, L.DD_DEV_NO_CHAINS)))
    assert ctx.lib.dd_dev_last_sample_chains(ctx.handle) == 1


@pytest.mark.parametrize("hold", [0, 3])
@pytest.mark.parametrize("D,H", [(768, 12), (1024, 16)])
def test_real_exit_on_the_gemm_path_widths(D, H, hold):
    """Case D: the widths without a fused block tail (row-resident and split-K Linears), depth 5, 256 patches, B = 3; exits on the first
    layers, and on the out-blocks (layers 3 and 4)."""
    mpd = dict(img_size=32, patch_size=2, in_chans=3, embed_dim=D, depth=5, num_heads=H, mlp_ratio=4, qkv_bias=False,
               mlp_time_embed=False, num_classes=-1, normalize_timesteps=True)
    m, mp = _engine(mpd, 78, "mlp_probe_per_layer", "bf16", max_batch=3, hold=hold)
    _check_case(m, mp, 3, 2, _pick_threshold(m, mp, 3, 2, seed=6, hold=hold))


# ---------------------------------------------------------------- 2. the reference's decisions
@pytest.mark.parametrize("tag", ["thr45", "thr39", "thr100"])
def test_real_exit_rollout_at_the_reference_thresholds(tag):
    """The model, the batch and the thresholds of the reference rollout fixture (ee_rollout.npz), fp32, all 1000 steps.  The fixture's own
    trajectory is drawn from the torch CPU stream, which no device loop can follow (test_engine_rollout_vs_reference pins the host-noise
    path to it); the real-exit loop draws on the device, so it is compared with the simulated device loop on the same seed: every one of
    the 3000 exit indices, and the images."""
    roll = np.load(GOLDEN / "ee_rollout.npz")
    m, mp = _engine(dict(TINY), int(roll["seed_model"]), "mlp_probe_per_layer", "fp32")
    thr = float(roll[f"{tag}_threshold"])
    want, w_ind = _run(m, mp, 3, thr, "device", 1000)
    got, g_ind = _run(m, mp, 3, thr, "device_real", 1000)
    flips = int((g_ind != w_ind).sum())
    assert flips == 0, f"{flips} exit decisions differ"
    assert np.array_equal(got, want)


# ---------------------------------------------------------------- 3. it really skips
def _skipping_setup():
    """A TINY model and a threshold chosen on the SIMULATED loop alone (B = 6, one chain, 60 steps): more than one exit is taken, at least
    one step needs a move (an exited slot in front of a surviving one) and at least one needs none."""
    from duodiff_amd import _lib as L
    B, steps = 6, 60
    for seed in (91, 92, 93, 94, 95, 96):
        m, mp = _engine(dict(TINY), seed, "mlp_probe_per_layer", "fp32")
        ctx = m.engine_model(B).ctx
        cls0 = np.sort(_first_cls(m, mp, B).numpy().ravel())
        for thr in ((cls0[:-1] + cls0[1:]) / 2)[2::3]:
            with dev_flags(ctx, L.DD_DEV_NO_CHAINS):
                want, w_ind = _run(m, mp, B, float(thr), "device", steps)
            per_step = [_moves_of_step(list(r), mp.depth, 1)[1] for r in w_ind.numpy().astype(int)]
            if len(set(w_ind.flatten().tolist())) > 1 and max(per_step) > 0 and min(per_step) == 0:
                return m, mp, ctx, B, steps, float(thr), want, w_ind
    raise AssertionError("no threshold among the candidates makes the simulated loop take more than one exit with and without moves")


def test_real_exit_runs_fewer_block_rows():
    from duodiff_amd import _lib as L
    m, mp, ctx, B, steps, thr, want, w_ind = _skipping_setup()
    depth, full = mp.depth, steps * B * mp.depth
    for s in (1, 2, depth + 1):
        for flags, halves in ((L.DD_DEV_NO_CHAINS, [(0, B)]), (L.DD_DEV_FORCE_CHAINS, [(0, B // 2), (B // 2, B)])):
            st = {}
            with dev_flags(ctx, flags):
                got, g_ind = _run(m, mp, B, thr, "device_real", steps, compact_every=s, stats=st)
            assert np.array_equal(got, want) and torch.equal(g_ind, w_ind)
            rows, moves = _expected(w_ind, depth, s, halves)
            print(f"compact_every {s} chains {len(halves)}: block-rows {st['block_rows']} of {full}, moves {st['moves']}, compactions {st['compactions']}")
            assert st["block_rows_full"] == full
            assert st["block_rows"] == real_exit_block_rows(w_ind, depth, s) == rows
            assert st["moves"] == moves and (st["compactions"] > 0) == (moves > 0)
            if s <= depth:
                assert st["block_rows"] < full
            if len(halves) == 1 and s == 1:
                assert st["moves"] > 0
    # compact_every = depth + 1: layer 0 is the one compaction layer (0 % s == 0), so only the images that leave at layer 0 are dropped:
    # with none of those, the loop launches every block on every image
    at0 = int((w_ind == 0).sum())
    assert real_exit_block_rows(w_ind, depth, depth + 1) == full - depth * at0


def test_real_exit_that_never_compacts_runs_every_block():
    """compact_every = depth + 1 compacts at layer 0 alone.  Layer 0's probe is given a bias of +30 (its prediction is 1 to the last bit,
    above the threshold), so no image leaves there while the layers behind it keep their exits: block-rows == steps * B * depth."""
    from duodiff_amd.early_exit import EarlyExitUViT
    from duodiff_amd.uvit import UViT
    B, steps = 6, 40
    mp = ModelParams.from_dict(dict(TINY))
    sd = synthetic_ee_state_dict(mp, 91, "mlp_probe_per_layer")
    sd["matrix.0.classifier.0.bias"] = sd["matrix.0.classifier.0.bias"] + 30.0
    m = EarlyExitUViT(UViT(**mp.as_dict(), precision="fp32"), "mlp_probe_per_layer")
    m.load_state_dict(sd).eval().to("cuda")
    thr = float(_first_cls(m, mp, B)[1:].median())
    want, w_ind = _run(m, mp, B, thr, "device", steps)
    assert int((w_ind == 0).sum()) == 0 and len(set(w_ind.flatten().tolist())) > 1
    st = {}
    got, g_ind = _run(m, mp, B, thr, "device_real", steps, compact_every=mp.depth + 1, stats=st)
    assert np.array_equal(got, want) and torch.equal(g_ind, w_ind)
    assert st["block_rows"] == steps * B * mp.depth and st["moves"] == 0


# ---------------------------------------------------------------- 4. edge thresholds
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_real_exit_edge_thresholds(precision):
    B, steps = 6, 30
    m, mp = _engine(dict(TINY), 91, "mlp_probe_per_layer", precision)
    for thr, rows in ((float("inf"), 0), (1e-30, steps * B * mp.depth)):      # (an MLP probe is a mean of sigmoids: > 1e-30)
        want, w_ind = _run(m, mp, B, thr, "device", steps)
        assert set(w_ind.flatten().tolist()) == ({0.0} if rows == 0 else {float(mp.depth)})
        for s in (1, 2):
            st = {}
            got, g_ind = _run(m, mp, B, thr, "device_real", steps, compact_every=s, stats=st)
            assert np.array_equal(got, want) and torch.equal(g_ind, w_ind)
            assert st["block_rows"] == rows and st["moves"] == 0
    # a negative threshold no prediction passes: the reference's argmax of an all-False column is 0, so every image takes head 0's output --
    # after it has run every block (a later layer might have passed)
    want, w_ind = _run(m, mp, B, -1.0, "device", steps)
    st = {}
    got, g_ind = _run(m, mp, B, -1.0, "device_real", steps, stats=st)
    assert set(w_ind.flatten().tolist()) == {0.0} and np.array_equal(got, want) and torch.equal(g_ind, w_ind)
    assert st["block_rows"] == steps * B * mp.depth


# ---------------------------------------------------------------- 5. poison
def test_real_exit_reads_no_stale_slab(case_b):
    """Every activation buffer filled with NaN bytes right before the call: a slab read after a move that did not carry it shows as NaN."""
    from duodiff_amd import _lib as L
    tm, tmp_, tctx, tB, tsteps, tthr, twant, tind = _skipping_setup()
    for m, mp, B, steps, thr, want, w_ind, flags in ((*case_b[:2], 7, 3, *case_b[2], L.DD_DEV_NO_CHAINS), (tm, tmp_, tB, tsteps, tthr, twant, tind, L.DD_DEV_NO_CHAINS),
                                                     (tm, tmp_, tB, tsteps, tthr, twant, tind, L.DD_DEV_FORCE_CHAINS)):
        em = m.engine_model(B)
        ctx = em.ctx
        with dev_flags(ctx, flags):
            st = {}
            ctx.check(ctx.lib.dd_dev_poison_workspaces(ctx.handle, em.handle, torch.cuda.current_stream().cuda_stream))
            got, g_ind = _run(m, mp, B, thr, "device_real", steps, stats=st)
        assert flags == L.DD_DEV_FORCE_CHAINS or st["moves"] > 0, "the run should move slabs"
        assert np.isfinite(got).all() and np.array_equal(got, want) and torch.equal(g_ind, w_ind)


# ---------------------------------------------------------------- 6. rejections and the CLI
def test_real_exit_rejections():
    from duodiff_amd import _lib as L
    from duodiff_amd.engine import sample_early_exit_real_loop
    from duodiff_amd.uvit import UViT
    m, mp = _engine(dict(TINY), 91, "mlp_probe_per_layer", "fp32")
    em = m.engine_model(3)
    ctx = em.ctx
    x = torch.randn(3, 3, 8, 8, device="cuda")
    before = x.clone()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(model=em, noise=L.DD_NOISE_PHILOX, err=None, real=L.dd_ee_real(1, 0)):
        a = L.dd_ee_sample_args()
        a.model, a.threshold, a.t_start, a.t_end, a.noise_mode, a.B, a.x_dev = model.handle, 0.4, 999, 990, noise, 3, x.data_ptr()
        a.err_dev = err.data_ptr() if err is not None else None
        rc = ctx.lib.dd_sample_early_exit_real(ctx.handle, C.byref(a), C.byref(real) if real is not None else None, stream)
        return rc, (ctx.lib.dd_last_error(ctx.handle) or b"").decode()

    u = UViT(**mp.as_dict(), precision="fp32").load_state_dict(synthetic_state_dict(mp, 1)).to("cuda")
    rc, msg = call(model=u.engine_model(3))
    assert rc == L.DD_ERR_STATE and "early_exit" in msg
    rc, msg = call(real=L.dd_ee_real(0, 0))
    assert rc == L.DD_ERR_INVALID and "compact_every" in msg
    rc, msg = call(noise=L.DD_NOISE_BUFFER)
    assert rc == L.DD_ERR_INVALID and "noise" in msg
    rc, msg = call(real=None)
    assert rc == L.DD_ERR_INVALID and "dd_ee_real" in msg
    rc, msg = call(err=torch.zeros(1000, mp.depth, device="cuda"))
    assert rc == L.DD_ERR_INVALID and "err_dev" in msg
    torch.cuda.synchronize()
    assert torch.equal(x, before), "a rejected call must not have enqueued anything"
    assert call()[0] == L.DD_OK
    with pytest.raises(ValueError, match="compact_every"):
        sample_early_exit_real_loop(ctx, em, x, 0.4, compact_every=0)
    with pytest.raises(ValueError, match="err"):
        sample_early_exit_real_loop(ctx, em, x, 0.4, err=torch.zeros(1000, mp.depth, device="cuda"))


def test_real_exit_cli(tmp_path):
    """--real_exit writes the PNG bytes and the indices --noise device writes, and the block-rows into statistics.txt."""
    import subprocess, sys, yaml
    cfg = dict(TINY)
    mp = ModelParams.from_dict(cfg)
    (tmp_path / "m.yaml").write_text(yaml.safe_dump({"model_params": dict(cfg, classifier_type="mlp_probe_per_layer")}))
    torch.save({"model_state_dict": dict(synthetic_ee_state_dict(mp, 41, "mlp_probe_per_layer"))}, tmp_path / "m.pth")
    base = [sys.executable, "-m", "duodiff_amd.eesampler", "--seed", "5", "--threshold", "0.39", "--checkpoint_path", str(tmp_path / "m.pth"),
            "--config_path", str(tmp_path / "m.yaml"), "--batch_size", "4", "--precision", "fp32"]
    for name, extra in (("sim", ["--noise", "device"]), ("real", ["--real_exit", "--compact_every", "2"])):
        r = subprocess.run(base + ["--output_folder", str(tmp_path / name)] + extra, cwd=str(REPO), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
    pngs = sorted(p.name for p in (tmp_path / "sim").glob("*.png"))
    assert len(pngs) >= 4 and pngs == sorted(p.name for p in (tmp_path / "real").glob("*.png"))
    for p in pngs:
        assert (tmp_path / "sim" / p).read_bytes() == (tmp_path / "real" / p).read_bytes(), p
    ind = torch.load(tmp_path / "real" / "indices_by_timestep.pt")
    assert torch.equal(ind, torch.load(tmp_path / "sim" / "indices_by_timestep.pt"))
    stats = (tmp_path / "real" / "statistics.txt").read_text().splitlines()
    rows = real_exit_block_rows(ind, mp.depth, 2)
    assert stats[0].startswith("Elapsed time: ") and stats[1] == f"Block rows run: {rows} of {1000 * 4 * mp.depth} ({rows / (1000 * 4 * mp.depth):.4f})"
