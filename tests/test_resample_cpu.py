"""Resampling jumps on the host (no GPU): the walk over a plan's grid (step_plan.walk_moves, RePaint's schedule and Restart's intervals as
its jumps), the rows of a walk plan (jump coefficients, late rows, saves, lands), predict_noise DDPM as affine rows, the rejected
combinations, the command line's validation and the binding.
"""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import REPO, TINY
from duodiff_amd import _lib as L
from duodiff_amd import step_plan as sp
from duodiff_amd.engine import schedule_tables
from loop_support import cli_argv

SCHEDULES = [(250, 10, 10), (1000, 10, 10), (50, 5, 3), (7, 7, 3), (6, 1, 3), (8, 3, 2)]
COUNTS = {(250, 10, 10): (2410, 216), (1000, 10, 10): (9910, 891), (50, 5, 3): (140, 18), (7, 7, 3): (7, 0)}


def _published_times(t_T, jump_length, jump_n_sample):
    """get_schedule_jump of the RePaint code (guided_diffusion/scheduler.py), transcribed: the times a run visits, from t_T - 1 down to -1,
    going back up jump_length steps wherever a time still has resamplings left"""
    jumps = {}
    for j in range(0, t_T - jump_length, jump_length):
        jumps[j] = jump_n_sample - 1
    t = t_T
    ts = []
    while t >= 1:
        t = t - 1
        ts.append(t)
        if jumps.get(t, 0) > 0:
            jumps[t] = jumps[t] - 1
            for _ in range(jump_length):
                t = t + 1
                ts.append(t)
    ts.append(-1)
    return ts


def _published_moves(n, j, r):
    """the published schedule as moves over positions p = n - 1 - t (time t_T - 1 is position 0, time -1 the final image): a descent of
    one is a step at the position it leaves, a run of j ascents one jump"""
    ts = _published_times(n, j, r)
    moves, i = [], 0
    while i + 1 < len(ts):
        p = n - 1 - ts[i]
        if ts[i + 1] == ts[i] - 1:
            moves.append(("S", p))
            i += 1
        else:
            assert ts[i + 1:i + 1 + j] == list(range(ts[i] + 1, ts[i] + j + 1))
            moves.append(("J", p, p - j))
            i += j
    return moves


@pytest.mark.parametrize("njr", SCHEDULES)
def test_walk_reproduces_the_published_schedule(njr):
    n, j, r = njr
    moves = sp.walk_moves(n, sp.repaint_jumps(n, j, r))
    assert moves == _published_moves(n, j, r)
    steps, jumps = sum(m[0] == "S" for m in moves), sum(m[0] == "J" for m in moves)
    assert steps == n + j * jumps
    if njr in COUNTS:
        assert (steps, jumps) == COUNTS[njr]
    assert all(1 <= m[1] < n and m[2] >= 0 for m in moves if m[0] == "J"), "a jump from the final image or past the start"


def test_walk_6_2_2_literally():
    S, J = (lambda p: ("S", p)), (lambda p, q: ("J", p, q))
    assert sp.walk_moves(6, sp.repaint_jumps(6, 2, 2)) == [S(0), S(1), S(2), J(3, 1), S(1), S(2), S(3), S(4), J(5, 3), S(3), S(4), S(5)]
    assert sp.walk_moves(6, {3: (2, 1), 5: (2, 1)}) == sp.walk_moves(6, sp.repaint_jumps(6, 2, 2))
    assert sp.walk_moves(3, {}) == [S(0), S(1), S(2)]
    # budgets never refill: position 2 is passed three times and jumps twice
    assert sp.walk_moves(4, {2: (1, 2), 3: (3, 1)}) == [S(0), S(1), J(2, 1), S(1), J(2, 1), S(1), S(2), J(3, 0), S(0), S(1), S(2), S(3)]
    for bad in ({0: (1, 1)}, {4: (1, 1)}, {2: (3, 1)}, {2: (0, 1)}, {2: (1, -1)}):
        with pytest.raises(ValueError):
            sp.walk_moves(4, bad)


def test_restart_snaps_to_the_grid():
    """a 10-point DDIM grid: the model sees 999, 888, ..., 111 and the last step lands on 0"""
    base = sp.step_plan(None, use_ddim=True, ddim_steps=10)
    levels = base.rows["t"].tolist()
    assert levels == [999.0, 888.0, 777.0, 666.0, 555.0, 444.0, 333.0, 222.0, 111.0]
    assert sp.restart_jumps(levels, [(200, 600, 3)]) == {7: (3, 3)}             # 222 is the smallest level >= 200, 555 the largest <= 600
    assert sp.restart_jumps(levels, [(222, 555, 1)]) == {7: (3, 1)}             # the ends themselves
    assert sp.restart_jumps(levels, [(100, 350, 2), (400, 1000, 1)]) == {8: (2, 2), 5: (5, 1)}
    assert sp.restart_jumps(levels, [(100, 444, 2), (444, 700, 1)]) == {8: (3, 2), 5: (2, 1)}      # two intervals may share one grid point
    p = sp.step_plan(None, use_ddim=True, ddim_steps=10, restart=[(200, 600, 2)])
    assert [m for m in p.moves if m[0] == "J"] == [("J", 7, 4)] * 2
    assert len(p.rows["t"]) == 9 + 2 * (3 + 1) and p.rows["jump"].sum() == 2
    for bad, match in (([(230, 330, 1)], "fewer than two"), ([(500, 560, 1)], "fewer than two"), ([(1000, 1200, 1)], "fewer than two"),
                       ([(0, 50, 1)], "fewer than two"), ([(100, 500, 1), (300, 700, 1)], "overlaps"), ([(300, 200, 1)], "t_min < t_max"),
                       ([(200, 600, 0)], "at least 1"), ([(200, 600)], "t_min, t_max, K")):
        with pytest.raises(ValueError, match=match):
            sp.step_plan(None, use_ddim=True, ddim_steps=10, restart=bad)


def test_rejected_combinations():
    ddim = dict(parametrization=None, use_ddim=True, ddim_steps=7)
    cases = [(dict(ddim, resample_jump=2), "go together"), (dict(ddim, resample_count=2), "go together"),
             (dict(ddim, resample_jump=2, resample_count=2, restart=[(100, 500, 1)]), "exclusive"),
             (dict(ddim, resample_jump=2, resample_count=0), "resample_count"), (dict(ddim, resample_jump=2, resample_count=-3), "resample_count"),
             (dict(ddim, resample_jump=0, resample_count=2), "resample_jump"), (dict(ddim, resample_jump=-1, resample_count=2), "resample_jump"),
             (dict(parametrization="predict_noise", solver="dpmsolver++", resample_jump=2, resample_count=2), "DPM-Solver"),
             (dict(parametrization="predict_noise", solver="sde-dpmsolver++", restart=[(100, 500, 1)]), "DPM-Solver"),
             (dict(parametrization="predict_noise", threshold=object(), resample_jump=2, resample_count=2), "thresholding"),
             (dict(ddim, threshold=object(), restart=[(100, 500, 1)]), "thresholding")]
    for kw, match in cases:
        with pytest.raises(ValueError, match=match):
            sp.step_plan(**kw)


def test_get_samples_rejects_pag_and_early_exit_before_any_engine_call():
    """the two rejections that need the models: _resolve_options raises before it touches one"""
    from duodiff_amd import sampler

    class Plain:
        depth, device = 3, "cpu"

    class EarlyExit(Plain):
        classifier_type = "attention_probe"

    def resolve(model, pag=None):
        plan_args = ("predict_noise", (), False, np.inf, 1000, True, 7, 0.0, None, 20, 2, None, None, 2, 2, None)
        return sampler._resolve_options(model, None, 2, (3, 8, 8), plan_args, "device", None, None, None, 1000, None, None, pag, None, None, None,
                                        None, None, None, walk=True)
    with pytest.raises(ValueError, match="perturbed-attention"):
        resolve(Plain(), pag=(1.0, [1], []))
    with pytest.raises(ValueError, match="early-exit"):
        resolve(EarlyExit())
    assert resolve(Plain())[0].moves


PLAN_CALLS = [dict(parametrization="predict_noise"), dict(parametrization="predict_noise", has_late=True, t_switch=300, timesteps_save=[500, 1000]),
              dict(parametrization="predict_noise", num_steps=20, strength=0.5), dict(parametrization="predict_original", has_late=True, t_switch=1),
              dict(parametrization="predict_previous", timesteps_save=[10]), dict(parametrization=None, use_ddim=True),
              dict(parametrization="predict_noise", use_ddim=True, ddim_steps=20, ddim_eta=0.01, has_late=True, t_switch=700, strength=0.3),
              dict(parametrization="predict_noise", solver="dpmsolver++", solver_steps=10, has_late=True, t_switch=300),
              dict(parametrization="predict_original", solver="sde-dpmsolver++", solver_order=1),
              dict(parametrization="predict_noise", threshold=object()), dict(parametrization="predict_noise", use_ddim=True, threshold=object())]


def _same_plan(p, q):
    assert (p.kind, p.save_after, p.switch_after, p.lands, p.moves) == (q.kind, q.save_after, q.switch_after, q.lands, q.moves)
    assert sorted(p.rows) == sorted(q.rows)
    for k in p.rows:
        assert p.rows[k].dtype == q.rows[k].dtype and p.rows[k].tobytes() == q.rows[k].tobytes(), k


@pytest.mark.parametrize("kw", PLAN_CALLS, ids=[str(i) for i in range(len(PLAN_CALLS))])
def test_plans_without_jumps_are_what_they_were(kw):
    """the new arguments left out, or None: the plan of today -- no jump / late rows, no moves"""
    p = sp.step_plan(**kw)
    assert p.moves == () and "jump" not in p.rows and "late" not in p.rows
    assert len(sp.StepPlan._fields) == 6 and sp.StepPlan._fields[:5] == ("kind", "rows", "save_after", "switch_after", "lands")
    _same_plan(sp.step_plan(**kw, resample_jump=None, resample_count=None, restart=None), p)
    _same_plan(sp.step_plan(**kw, restart=[]), p)


@pytest.mark.parametrize("kw", PLAN_CALLS[:7], ids=[str(i) for i in range(7)])
def test_r_one_and_long_jumps_give_the_jump_free_plan(kw):
    p = sp.step_plan(**kw)
    n = len(p.rows["t"])
    _same_plan(sp.step_plan(**kw, resample_jump=3, resample_count=1), p)
    _same_plan(sp.step_plan(**kw, resample_jump=n, resample_count=4), p)
    _same_plan(sp.step_plan(**kw, resample_jump=n + 7, resample_count=4), p)


def test_walk_rows_repeat_the_grid_rows():
    """a step row is the jump-free plan's row at its position, per visit; a jump row is (ja, 0, jc, 1); lands and saves follow the walk"""
    kw = dict(parametrization=None, use_ddim=True, ddim_steps=7, ddim_eta=0.01, timesteps_save=[501, 168, 2])
    base, p = sp.step_plan(**kw), sp.step_plan(**kw, resample_jump=2, resample_count=2)
    assert p.kind == "affine" and p.switch_after is None and list(p.moves) == sp.walk_moves(6, sp.repaint_jumps(6, 2, 2))
    assert all(len(v) == 12 for v in p.rows.values()) and len(p.save_after) == len(p.lands) == 12
    assert p.rows["jump"].dtype == p.rows["late"].dtype == np.int32 and p.rows["jump"].tolist() == [0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0]
    level = [int(t) for t in base.rows["t"]]
    ab = schedule_tables()["alphas_bar"].astype(np.float64)
    for k, mv in enumerate(p.moves):
        if mv[0] == "S":
            for key in ("t", "a", "b", "c", "noise"):
                assert p.rows[key][k] == base.rows[key][mv[1]], (k, key)
            assert p.lands[k] == base.lands[mv[1]]
        else:
            s, u = level[mv[1]], level[mv[2]]
            assert (p.rows["b"][k], p.rows["noise"][k], p.lands[k]) == (0.0, 1, u) and u > s
            assert p.rows["a"][k] == np.float32(np.sqrt(ab[u] / ab[s])) and p.rows["c"][k] == np.float32(np.sqrt(1.0 - ab[u] / ab[s]))
    ka, kb = sp.known_rows(p)                                   # a jump's row: the level it reaches (nothing reads it)
    assert ka[3] == np.float32(np.sqrt(ab[level[1]])) and kb[3] == np.float32(np.sqrt(1.0 - ab[level[1]])) and (ka[-1], kb[-1]) == (1.0, 0.0)
    # t = 499 (position 3) is visited at rows 6 and 9, t = 832 (position 1) at rows 1 and 4: the last visit is saved; 1000 - 2 is no grid point
    assert level[3] == 499 and level[1] == 832
    assert [k for k, s in enumerate(p.save_after) if s] == [4, 9]
    assert [k for k, s in enumerate(base.save_after) if s] == [1, 3]


def test_jump_coefficients():
    """ja^2 + jc^2 = 1 within 3 * 2^-24 (two roundings and the squares'); on the DDPM grid ja against sqrt(prod alpha_i) over the jumped
    steps within (j + 2) * 2^-23 relative (the tables are fp32: abar is a product of j rounded factors more, each half an ulp = 2^-24 relative
    at most, and the square root halves the sum; the bound leaves a factor 4)"""
    tb = schedule_tables()
    alphas = tb["alphas"].astype(np.float64)
    worst_unit, worst_prod = 0.0, 0.0
    for j, r in ((10, 3), (1, 2), (37, 2), (250, 2)):
        p = sp.step_plan("predict_noise", resample_jump=j, resample_count=r)
        level = 999 - np.arange(1000)
        jumps = [(k, mv) for k, mv in enumerate(p.moves) if mv[0] == "J"]
        assert len(jumps) == (r - 1) * len(sp.repaint_jumps(1000, j, r)) > 0
        for k, (_, pos, to) in jumps:
            ja, jc = float(p.rows["a"][k]), float(p.rows["c"][k])
            worst_unit = max(worst_unit, abs(ja * ja + jc * jc - 1.0))
            assert abs(ja * ja + jc * jc - 1.0) <= 3 * 2.0 ** -24
            s, u = level[pos], level[to]
            assert u - s == j
            want = np.sqrt(np.prod(alphas[s + 1:u + 1]))           # abar[u] / abar[s] = alpha_{s+1} ... alpha_u
            worst_prod = max(worst_prod, abs(ja - want) / want / ((j + 2) * 2.0 ** -23))
            assert abs(ja - want) <= (j + 2) * 2.0 ** -23 * want, (j, s, u)
    print(f"|ja^2 + jc^2 - 1| max {worst_unit / 2.0 ** -24:.2f} x 2^-24; ja vs sqrt(prod alpha) max {worst_prod:.3f} of the bound")
    assert sp.jump_coefficients(499, 499) == (1.0, 0.0)


@pytest.mark.parametrize("t_switch", [1, 300, 1000])
@pytest.mark.parametrize("kind", ["ddpm", "ddim"])
def test_late_rows_follow_the_jump_free_plan(kind, t_switch):
    """late[k] is what the jump-free plan runs at that grid position, under each sampler's own switch rule; the jumps cross the boundary
    upward (the walk returns to the first model) wherever it lies inside the grid"""
    kw = dict(parametrization="predict_noise", has_late=True, t_switch=t_switch)
    if kind == "ddim":
        kw.update(use_ddim=True, ddim_steps=21)
    base = sp.step_plan(**kw)
    n = len(base.rows["t"])
    sw = base.switch_after
    p = sp.step_plan(**kw, resample_jump=7 if t_switch == 300 else 3, resample_count=3)    # (lengths whose jumps straddle the boundary)
    steps =[(k, mv[1]) for k, mv in enumerate(p.moves) if mv[0] == "S"]
    for k, pos in steps:
        assert p.rows["late"][k] == int(sw is not None and pos >= sw), (k, pos)
    assert not p.rows["late"][p.rows["jump"] == 1].any()
    late = p.rows["late"][[k for k, _ in steps]]
    if sw is not None and 0 < sw < n:
        assert (np.diff(late) < 0).any(), "no jump crossed the switch upward"
    else:
        assert (late == int(sw == 0)).all()


def test_predict_noise_rows_against_the_engine_tables():
    """a = c1, b = -c1 c2 of dd_schedule_table within 4 * 2^-24 relative (c1 and c2 are two fp32 roundings each, the row one); c is sigma"""
    tb = schedule_tables()
    worst = 0.0
    for t in range(1000):
        a, b, c = sp.affine_coefficients("predict_noise", t)
        assert a.dtype == b.dtype == c.dtype == np.float32
        c1, c2 = float(tb["c1"][t]), float(tb["c2"][t])
        ea, eb = abs(float(a) - c1) / c1, abs(float(b) + c1 * c2) / (c1 * c2)
        worst = max(worst, ea, eb)
        assert ea <= 4 * 2.0 ** -24 and eb <= 4 * 2.0 ** -24, t
        assert abs(float(c) - float(tb["sigma"][t])) <= 2.0 ** -24 * float(tb["sigma"][t])
    print(f"predict_noise rows vs (c1, -c1 c2): max relative {worst / 2.0 ** -24:.2f} x 2^-24")
    # the walk plan of a DDPM run has them at every step row, and the jump-free "ddpm" kind is untouched
    p = sp.step_plan("predict_noise", num_steps=8, resample_jump=2, resample_count=2)
    assert p.kind == "affine" and sp.step_plan("predict_noise", num_steps=8).kind == "ddpm"
    k = [i for i, mv in enumerate(p.moves) if mv == ("S", 5)][-1]
    assert (p.rows["a"][k], p.rows["b"][k], p.rows["c"][k]) == sp.affine_coefficients("predict_noise", 994) and p.rows["t"][k] == 994


# ---- plumbing -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra,match", [
    (["--resample_jump", "2"], "go together"),
    (["--resample_count", "2"], "go together"),
    (["--resample_jump", "0", "--resample_count", "2"], "at least 1"),
    (["--resample_jump", "2", "--resample_count", "0"], "at least 1"),
    (["--resample_jump", "2", "--resample_count", "2", "--restart", "100", "500", "2"], "exclusive"),
    (["--restart", "100", "500", "0"], "at least 1"),
    (["--restart", "100", "500", "1.5"], "whole number"),
    (["--restart", "500", "100", "1"], "T_MIN < T_MAX"),
    (["--restart", "100", "1200", "1"], "T_MIN < T_MAX"),
    (["--use_ddim", "--ddim_steps", "10", "--restart", "230", "330", "1"], "fewer than two"),
    (["--use_ddim", "--ddim_steps", "10", "--restart", "100", "500", "1", "--restart", "300", "700", "1"], "overlaps"),
    (["--resample_jump", "2", "--resample_count", "2", "--dpm_solver", "ode"], "exclusive"),
    (["--restart", "100", "500", "1", "--dpm_solver", "sde"], "exclusive"),
    (["--resample_jump", "2", "--resample_count", "2", "--clip_x0"], "exclusive"),
    (["--resample_jump", "2", "--resample_count", "2", "--dynamic_threshold", "0.99"], "exclusive"),
    (["--resample_jump", "2", "--resample_count", "2", "--pag_scale", "1.0"], "exclusive"),
])
def test_cli_rejects_bad_resampling_options_before_any_gpu_work(tmp_path, extra, match):
    import yaml
    from duodiff_amd import dist, sampler
    (tmp_path / "m.yaml").write_text(yaml.safe_dump({"model_params": dict(TINY)}))
    argv = cli_argv(tmp_path / "m.yaml", *extra)
    with pytest.raises(ValueError, match=match):
        sampler.main(argv)                  # (the checkpoint does not exist: passing validation would fail differently)
    with pytest.raises(ValueError, match=match):
        dist.main(argv)


def test_cli_parses_the_resampling_options(tmp_path):
    import yaml
    from duodiff_amd import sampler
    (tmp_path / "m.yaml").write_text(yaml.safe_dump({"model_params": dict(TINY)}))
    a = sampler.get_args(cli_argv(tmp_path / "m.yaml"))
    assert (a.resample_jump, a.resample_count, a.restart) == (None, None, None)
    assert sampler.validate_resample(a) == dict(resample_jump=None, resample_count=None, restart=None)
    a = sampler.get_args(cli_argv(tmp_path / "m.yaml", "--use_ddim", "--resample_jump", "10", "--resample_count", "10"))
    assert sampler.validate_resample(a) == dict(resample_jump=10, resample_count=10, restart=None)
    a = sampler.get_args(cli_argv(tmp_path / "m.yaml", "--restart", "50", "300", "2", "--restart", "400", "800", "1"))
    assert sampler.validate_resample(a) == dict(resample_jump=None, resample_count=None, restart=[(50.0, 300.0, 2), (400.0, 800.0, 1)])


def test_lib_binds_the_walk_entry_points():
    assert L.ABI_VERSION == 6
    assert C.sizeof(L.dd_walk) == 16 and L.dd_walk.late.offset == 8
    assert L.SIGNATURES["dd_sample_affine_walk"] == (C.c_int, [C.c_void_p, C.POINTER(L.dd_affine_sample_args), C.POINTER(L.dd_guidance),
                                                                C.POINTER(L.dd_autoguidance), C.POINTER(L.dd_known_region), C.POINTER(L.dd_walk),
                                                                C.c_void_p])
    assert L.SIGNATURES["dd_jump_step"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_int64, C.c_void_p])
    header = (REPO / "include" / "duodiff.h").read_text()
    assert re.search(r"#define DD_ABI_VERSION 6\b", header)
    assert re.search(r"typedef struct dd_walk \{\s*const int32_t\* jump;[^}]*const int32_t\* late;[^}]*\} dd_walk;", header)
    for name in ("dd_sample_affine_walk", "dd_jump_step"):
        assert re.search(rf"int {name}\(dd_ctx\* ctx,", header)
    lib = L.load()
    assert lib.dd_abi_version() == 6 and hasattr(lib, "dd_sample_affine_walk") and hasattr(lib, "dd_jump_step")
    # a null context is refused: the symbols exist and check their arguments without a GPU
    assert lib.dd_jump_step(None, None, None, 1.0, 0.0, None, 0, None) == L.DD_ERR_INVALID
    assert lib.dd_sample_affine_walk(None, None, None, None, None, None, None) == L.DD_ERR_INVALID
