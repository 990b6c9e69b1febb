"""tests/loop_support.py without a GPU: the seeded draws against the expressions they replaced, the planner of a cut loop against
sampler._segment_models, and the calls loop_calls makes -- recorded on stand-ins for the engine's loop entries, the context and the stream --
against what the helpers it replaced passed, written out here.  (run_loop itself is loop_calls on copies of x and h inside
`with torch.cuda.stream(stream)`, which takes no stand-in on a machine with a GPU: the inner function is what is recorded.)"""
import contextlib
import itertools
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import loop_support as ls


# ---- the draws: the bytes of the expressions in the test files before ---------------------------------------------------------------
def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.numpy().tobytes() == b.numpy().tobytes()


@pytest.mark.parametrize("B,C,S,seed", [(4, 3, 8, 2), (6, 3, 8, 3), (32, 3, 64, 4), (6, 3, 16, 5), (128, 3, 64, 7), (32, 4, 32, 12), (2, 3, 64, 35),
                                        (6, 3, 16, 2)])
def test_images_are_the_draws_they_replace(B, C, S, seed):
    assert same(ls.draw_images(B, C, S, seed), torch.randn(B, C, S, S, generator=torch.Generator().manual_seed(seed)))
    # test_x0_threshold._start
    assert same(ls.draw_images(B, C, S, seed, scale=1.0), torch.randn(B, C, S, S, generator=torch.Generator().manual_seed(seed)) * 1.0)
    assert same(ls.draw_images(B, C, S, seed, scale=2.5), torch.randn(B, C, S, S, generator=torch.Generator().manual_seed(seed)) * 2.5)


@pytest.mark.parametrize("B,ncls,seed", [(6, 10, 8), (4, 10, 10), (32, 10, 12), (6, 10, 6), (6, 10, 4), (32, 1000, 12), (4, 10, 18)])
def test_labels_are_the_draws_they_replace(B, ncls, seed):
    want = torch.randint(0, ncls, (B,), generator=torch.Generator().manual_seed(seed))
    assert same(ls.draw_labels(B, ncls, seed), want) and want.dtype == torch.int64


@pytest.mark.parametrize("B,seed,S,mask", [(2, 33, 8, "checker"), (6, 34, 8, "checker"), (32, 42, 64, "checker"), (3, 62, 8, "half"), (2, 31, 8, 0.0),
                                           (2, 32, 8, 1.0)])
def test_region_inputs_are_the_draws_they_replace(B, seed, S, mask):
    """test_known_region._inputs, which test_resample._inputs repeated without the constant mask: x, then x0, from one generator"""
    g = torch.Generator().manual_seed(seed)
    x, x0 = torch.randn(B, 3, S, S, generator=g), torch.randn(B, 3, S, S, generator=g)
    if mask == "checker":
        i = torch.arange(S)
        m = ((i[:, None] + i[None, :]) % 2).float().expand(B, 1, S, S).clone()
        m[:, :, 1::3, ::2] = 0.5
        m[B - 1] = 1 - m[B - 1]
    elif mask == "half":
        m = torch.zeros(B, 1, S, S)
        m[..., : S // 2] = 1
    else:
        m = torch.full((B, 1, S, S), float(mask))
    got = ls.draw_region_inputs(B, seed, S=S, mask=mask)
    assert all(same(a, b) for a, b in zip(got, (x, x0, m)))
    if mask == "checker":
        assert set(m.unique().tolist()) == {0.0, 0.5, 1.0} and not torch.equal(m[0], m[B - 1])


def test_step_tables():
    r = ls.ddpm_rows(4)
    assert r["t"].tolist() == [999.0, 998.0, 997.0, 996.0] and r["noise"].tolist() == [1, 1, 1, 1]
    assert ls.ddpm_rows(3, 2)["t"].tolist() == [2.0, 1.0, 0.0] and ls.ddpm_rows(3, 2)["noise"].tolist() == [1, 1, 0]
    a = ls.affine_rows(5)
    assert a["t"].tolist() == [999.0, 998.0, 997.0, 996.0, 995.0] and (a["c"] > 0).all() and a["a"].dtype == np.float32
    assert sorted(ls.ms_rows(6)) == sorted(["t", "a", "b", "c", "d", "p", "q", "hist", "noise"]) and len(ls.ms_rows(6)["t"]) == 6


# ---- the planner --------------------------------------------------------------------------------------------------------------------
def cut_sets(n):
    rows = range(1, n)
    return [()] + [(c,) for c in rows] + list(itertools.combinations(rows, 2))


def test_planner_agrees_with_the_samplers_segment_models():
    """every n <= 6, every switch_after in {None, 0 .. n}, every set of at most two cuts"""
    from duodiff_amd import sampler
    seen = 0
    for n in range(1, 7):
        for switch_after in [None, *range(n + 1)]:
            plan = NS(switch_after=switch_after)
            for cuts in cut_sets(n):
                segs = list(ls.loop_segments(n, cuts, switch_after))
                assert [s[0] for s in segs] == [0, *cuts] and [s[1] for s in segs] == [*cuts, n]
                for k0, k1, sw in segs:
                    want = sampler._segment_models(plan, k0, k1, "first", "late")
                    assert (*ls.segment_models("first", "late", sw, k1 - k0), sw) == want, (n, switch_after, cuts, k0, k1)
                    seen += 1
    assert seen == sum((n + 2) * sum(len(c) + 1 for c in cut_sets(n)) for n in range(1, 7)) > 600


def test_the_two_conventions_of_cuts():
    """test_block_cache._device cut AFTER the steps in cuts (its edges: c + 1); every other helper started a new call AT the rows in cuts"""
    for n in range(2, 7):
        for cuts in cut_sets(n - 1):
            after = [0, *[c + 1 for c in cuts], n]                                      # _device's edges
            segs = list(ls.loop_segments(n, [c + 1 for c in cuts]))
            assert [s[0] for s in segs] + [n] == after and [s[1] for s in segs] == after[1:]
    assert [(k0, k1) for k0, k1, _ in ls.loop_segments(7, (2, 3, 6))] == [(0, 2), (2, 3), (3, 6), (6, 7)]      # test_known_region's cuts


# ---- the calls of the driver ----------------------------------------------------------------------------------------------------------
ENTRIES = ["sample_loop", "sample_region_loop", "sample_affine_loop", "sample_affine_region_loop", "sample_multistep_loop",
           "sample_multistep_region_loop", "sample_multistep_threshold_loop", "sample_affine_walk_loop", "sample_affine_cached_loop"]
N, FLAGS = 6, 5
ROWS = {k: np.arange(N, dtype=np.float32) + 10 * i for i, k in enumerate("tabcdpq")}
ROWS["t"] = np.arange(N - 1, -1, -1, dtype=np.float32)
ROWS.update(noise=np.array([1, 1, 1, 1, 1, 0], np.int32), hist=np.array([0, 1, 1, 1, 1, 0], np.int32))
KA, KB = np.arange(N, dtype=np.float32) + 100, np.arange(N, dtype=np.float32) + 200


@pytest.fixture
def rig(monkeypatch):
    """(log, ctx, stream, models A and B): the engine's loop entries, dd_dev_set_flags and image_seeds append to the log"""
    from duodiff_amd import engine
    log = []

    @contextlib.contextmanager
    def image_seeds(seeds, stream):
        log.append(("seeds", seeds))
        yield
        log.append(("seeds", None))

    lib = NS(dd_dev_set_flags=lambda h, f: log.append(("flags", f)) or 0, dd_dev_last_sample_chains=lambda h: 2)
    ctx = NS(lib=lib, handle=7, check=lambda rc: None, image_seeds=image_seeds)
    for name in ENTRIES:
        monkeypatch.setattr(engine, name, lambda *a, _name=name, **kw: log.append((_name, a, kw)))
    stream = NS(synchronize=lambda: log.append(("synchronize",)))
    return log, ctx, stream, NS(ctx=ctx, name="A"), NS(ctx=ctx, name="B")


def entries(log):
    return [e for e in log if e[0] in ENTRIES]


def calls(log):
    """the recorded loop calls in the fields the old helpers differed in: (entry, first, late, row slices, region rows, the rest)"""
    out = []
    for name, a, kw in entries(log):
        region = kw.get("region") if "region" in kw else next((v for v in a if hasattr(v, "ka")), None)
        tables = next((v for v in a[4:] if isinstance(v, dict)), None)                    # (the affine entries take five arrays instead)
        tables = tables or dict(zip(("t", "a", "b", "c", "noise"), [v for v in a[4:] if isinstance(v, np.ndarray)]))
        rest = {k: kw[k] for k in ("counter_base", "switch_after", "t_start", "t_end", "t_switch", "blocks", "order") if k in kw}
        out.append((name, a[1].name, None if a[2] is None else a[2].name, {k: v.tolist() for k, v in tables.items()},
                    None if region is None else (region.ka.tolist(), region.kb.tolist()), rest))
    return out


def sl(k0, k1, keys):
    return {k: ROWS[k][k0:k1].tolist() for k in keys}


def region_of(with_region):
    from duodiff_amd.engine import KnownRegion
    return KnownRegion("x0", "mask", KA, KB) if with_region else None


def reg(with_region, k0, k1):
    return (KA[k0:k1].tolist(), KB[k0:k1].tolist()) if with_region else None


AFFINE, MULTISTEP = ("t", "a", "b", "c", "noise"), tuple(ROWS)
COMMON = dict(y="y", seed=11, noise="philox", use_graph=False, guidance="g")


def run(rig, kind, with_region, **kw):
    log, ctx, stream, A, B = rig
    rows = dict(ROWS, jump=np.zeros(N, np.int32)) if kind == "walk" else dict(ROWS, cache=np.zeros(N, np.int32), cw=ROWS["d"]) if kind == "cached" else ROWS
    chains = ls.loop_calls(kind, A, "x", "h", rows, stream, late=B, region=region_of(with_region), cuts=(2,), flags=FLAGS, **COMMON, **kw)
    assert chains == 2
    # the flags are set first and cleared last, the stream is synchronised behind the last call and inside the flags
    assert log[0] == ("flags", FLAGS) and log[-1] == ("flags", 0) and log[-3] == ("synchronize",) and log[-4][0] in ENTRIES
    for name, a, k in entries(log):
        assert a[0] is ctx and a[3] == "x" and k["stream"] is stream and all(k[key] == v for key, v in COMMON.items())
        assert any(isinstance(v, str) and v == "h" for v in a[4:]) == name.startswith("sample_multistep")
    return calls(log)


@pytest.mark.parametrize("with_region", [False, True])
def test_ddpm_calls(rig, with_region):
    """test_known_region._loop: both models whole, t_start / t_end from the call's t, no counter base (the timestep is the counter)"""
    entry = "sample_region_loop" if with_region else "sample_loop"
    assert run(rig, "ddpm", with_region, t_switch=997) == [
        (entry, "A", "B", {}, reg(with_region, 0, 2), dict(t_start=5, t_end=4, t_switch=997)),
        (entry, "A", "B", {}, reg(with_region, 2, 6), dict(t_start=3, t_end=0, t_switch=997))]


@pytest.mark.parametrize("with_region", [False, True])
def test_affine_calls(rig, with_region):
    """test_known_region._loop's affine call with test_multistep._loop's rule for the models: the switch at row 4 lies behind the first
    call (its late model is not passed) and two rows into the second"""
    entry = "sample_affine_region_loop" if with_region else "sample_affine_loop"
    assert run(rig, "affine", with_region, switch_after=4) == [
        (entry, "A", None, sl(0, 2, AFFINE), reg(with_region, 0, 2), dict(counter_base=0, switch_after=2)),
        (entry, "A", "B", sl(2, 6, AFFINE), reg(with_region, 2, 6), dict(counter_base=2, switch_after=2))]


@pytest.mark.parametrize("with_region", [False, True])
def test_multistep_calls(rig, with_region):
    """test_multistep._loop; a switch at row 2 = the cut: the late model starts the second call and is its only model"""
    entry = "sample_multistep_region_loop" if with_region else "sample_multistep_loop"
    assert run(rig, "multistep", with_region, switch_after=2) == [
        (entry, "A", None, sl(0, 2, MULTISTEP), reg(with_region, 0, 2), dict(counter_base=0, switch_after=2)),
        (entry, "B", None, sl(2, 6, MULTISTEP), reg(with_region, 2, 6), dict(counter_base=2, switch_after=0))]


@pytest.mark.parametrize("with_region", [False, True])
def test_threshold_calls(rig, with_region):
    """test_x0_threshold._loop: one entry, the region by keyword; no late model: no switch"""
    log, ctx, stream, A, _ = rig
    ls.loop_calls("threshold", A, "x", "h", ROWS, stream, threshold="thr", region=region_of(with_region), cuts=(2,), switch_after=4, **COMMON)
    assert calls(log) == [
        ("sample_multistep_threshold_loop", "A", None, sl(0, 2, MULTISTEP), reg(with_region, 0, 2), dict(counter_base=0, switch_after=None)),
        ("sample_multistep_threshold_loop", "A", None, sl(2, 6, MULTISTEP), reg(with_region, 2, 6), dict(counter_base=2, switch_after=None))]
    assert all(a[4] == "h" and a[6] == "thr" for name, a, _ in entries(log))
    assert log[0] == ("flags", 0) and log[-1] == ("flags", 0)
    # ... and without a threshold the kind is the plain multistep loop (thr None in the old helper)
    del log[:]
    ls.loop_calls("threshold", A, "x", "h", ROWS, stream, region=region_of(with_region), **COMMON)
    assert [c[0] for c in calls(log)] == ["sample_multistep_region_loop" if with_region else "sample_multistep_loop"]


@pytest.mark.parametrize("with_region", [False, True])
def test_walk_calls(rig, with_region):
    """test_resample._walk: the rows name their model, so both models go whole and switch_after - k0 unclamped"""
    keys = AFFINE + ("d", "p", "q", "hist", "jump")
    want = [("sample_affine_walk_loop", "A", "B", k0, k1, sw) for k0, k1, sw in ((0, 2, 1), (2, 6, -1))]
    got = run(rig, "walk", with_region, switch_after=1)
    assert [(c[0], c[1], c[2], c[4], c[5]) for c in got] == [
        (e, f, l, reg(with_region, k0, k1), dict(counter_base=k0, switch_after=sw)) for e, f, l, k0, k1, sw in want]
    assert [sorted(c[3]) for c in got] == [sorted(keys)] * 2 and [c[3]["t"] for c in got] == [[5.0, 4.0], [3.0, 2.0, 1.0, 0.0]]


@pytest.mark.parametrize("with_region", [False, True])
def test_cached_calls(rig, with_region):
    """test_block_cache._device (whose cuts=(1,) is cuts=(2,) here): sampler._segment_models' models, blocks and order by keyword"""
    got = run(rig, "cached", with_region, switch_after=4, cache=(2, 1))
    assert [(c[0], c[1], c[2], c[4], c[5]) for c in got] == [
        ("sample_affine_cached_loop", "A", None, reg(with_region, 0, 2), dict(counter_base=0, switch_after=2, blocks=2, order=1)),
        ("sample_affine_cached_loop", "A", "B", reg(with_region, 2, 6), dict(counter_base=2, switch_after=2, blocks=2, order=1))]
    assert [c[3]["cw"] for c in got] == [ROWS["d"][:2].tolist(), ROWS["d"][2:].tolist()]


def test_seeds_flags_and_failures(rig):
    log, ctx, stream, A, B = rig
    ls.loop_calls("affine", A, "x", "h", ROWS, stream, image_seeds=[3, 4], flags=FLAGS)
    assert [e for e in log if e[0] in ("flags", "seeds")] == [("flags", FLAGS), ("seeds", [3, 4]), ("seeds", None), ("flags", 0)]
    assert calls(log)[0][5] == dict(counter_base=0, switch_after=None)                    # (no late model: no switch)
    del log[:]
    with pytest.raises(ValueError, match="kind"):
        ls.loop_calls("euler", A, "x", "h", ROWS, stream, flags=FLAGS)
    assert log[0] == ("flags", FLAGS) and log[-1] == ("flags", 0), "a failing call left the flags set"


def test_a_region_beside_a_plan_takes_the_plans_rows(rig):
    """region=(x0, mask) with a StepPlan: sampler.known_rows of the plan, sliced per call (loop_support.known_region)"""
    from duodiff_amd import sampler
    log, ctx, stream, A, _ = rig
    plan = sampler.step_plan("predict_noise", strength=5 / 999)
    ka, kb = sampler.known_rows(plan)
    ls.loop_calls("ddpm", A, "x", "h", plan, stream, region=("x0", "mask"), cuts=(3,))
    got = calls(log)
    assert [c[4] for c in got] == [(ka[:3].tolist(), kb[:3].tolist()), (ka[3:].tolist(), kb[3:].tolist())]
    assert [c[5] for c in got] == [dict(t_start=5, t_end=3), dict(t_start=2, t_end=0)]
    assert all(a[4].x0 == "x0" and a[4].mask == "mask" for name, a, _ in entries(log))
