"""The host arithmetic of sampling: each sampler's update as per-step coefficient rows, and the StepPlan get_samples runs (timesteps,
rows, noise flags, save points, the late model's first step).  numpy and the engine's bit-exact schedule tables only: no torch, no GPU."""
from typing import NamedTuple, Optional

import numpy as np

from .engine import schedule_tables


def _f32(v):
    return np.float32(v)


def affine_coefficients(kind, t, s=None, eta=0.0):
    """Scalar (a, b, c) with x' = a*x + b*model_output + c*z for the reference's other updates, in fp32
    from the engine's (bit-exact) tables:
      "predict_original"  sampler.py:59-72      "predict_previous"  sampler.py:75-79
      "ddim" (t -> s)     sampler.py:112-120 (noise scaled by sigma^2 = betas_tilde[t]*eta, as the reference does)
      "predict_noise"     sampler.py:47-56 as a table row (the walk plans: resampling jumps need a table-driven loop), formed as
                          unfolded_rows forms its rows -- float64 from the tables, each coefficient rounded once:
                          a = 1 / sqrt(alpha_t), b = -beta_t / (sqrt(alpha_t) sqrt(1 - abar_t)), c = sqrt(betas_tilde[t]), with
                          beta_t = 1 - alpha_t from the alphas table, as the DDPM kernel's c2 has it (the betas table differs
                          from it by alpha's rounding, 2^-25 absolute: 3e-4 of beta_0)
    """
    tb = schedule_tables()
    one = _f32(1)
    if kind == "predict_noise":
        al, ab = float(tb["alphas"][t]), float(tb["alphas_bar"][t])
        return _f32(1.0 / np.sqrt(al)), _f32(-(1.0 - al) / (np.sqrt(al) * np.sqrt(1.0 - ab))), _f32(np.sqrt(float(tb["betas_tilde"][t])))
    if kind == "predict_previous":
        return _f32(0), one, np.sqrt(tb["betas_tilde"][t])
    if kind == "predict_original":
        a_t, ab_t, ab_p, b_t = tb["alphas"][t], tb["alphas_bar"][t], tb["alphas_bar_previous"][t], tb["betas"][t]
        a = _f32(np.sqrt(a_t) * (one - ab_p)) / (one - ab_t)
        b = _f32(np.sqrt(ab_p) * b_t) / (one - ab_t)
        return _f32(a), _f32(b), np.sqrt(tb["betas_tilde"][t])
    if kind == "ddim":
        ab = tb["alphas_bar"]
        sig2 = _f32(tb["betas_tilde"][t] * _f32(eta))
        a = np.sqrt(_f32(ab[s] / ab[t]))
        b = _f32(np.sqrt(_f32(one - ab[s] - sig2)) - _f32(a * np.sqrt(_f32(one - ab[t]))))
        return _f32(a), b, sig2
    raise ValueError(kind)


MULTISTEP_KINDS = ("dpmsolver++", "sde-dpmsolver++")


def multistep_rows(kind, alphas_bar, order=2, parametrization="predict_noise", lower_order_final=True, unfolded=False):
    """float64 DPM-Solver++ (Lu et al., 2022) rows of the multistep update, for the steps alphas_bar[k] -> alphas_bar[k + 1]
    (len(alphas_bar) = N + 1 values of abar along the grid; the model sees the first N):

        x' = a x + b m [+ d h  if hist]  [+ c z  if noise]        h' = p x + q m

    m: the model output at step k, h: the previous step's data prediction x0 = p x + q m.  kind: "dpmsolver++" (ODE, no noise)
    or "sde-dpmsolver++" (the midpoint 2M SDE: every row here has noise = 1; multistep_coefficients drops the z of a step landing on
    t = 0).  order 2: step 0 is first order (no history yet), and with lower_order_final the last step too (on the product grid it
    lands on t = 0, where lambda jumps: a second-order step there extrapolates with r ~ 0.2 and overshoots).
    unfolded: the rows of the thresholded loop, x' = a x + b xh + ..., xh = the thresholded data prediction p x + q m: a = A,
    b = phi w0 (the default folds x0 into them: a = A + phi w0 p, b = phi w0 q).
    Returns a dict of float64 arrays a, b, c, d, p, q and int32 arrays hist, noise."""
    if kind not in MULTISTEP_KINDS:
        raise ValueError(f"solver must be one of {MULTISTEP_KINDS}, not {kind!r}")
    if order not in (1, 2):
        raise ValueError("solver order must be 1 or 2")
    if parametrization == "predict_previous":
        raise ValueError("DPM-Solver++ needs a model that predicts the noise or the data (predict_noise / predict_original), "
                         "not predict_previous")
    if parametrization not in ("predict_noise", "predict_original"):
        raise ValueError(parametrization)
    ab = np.asarray(alphas_bar, np.float64)
    n = len(ab) - 1
    if n < 1:
        raise ValueError("need at least one step")
    alpha, sigma = np.sqrt(ab), np.sqrt(1.0 - ab)
    lam = np.log(alpha) - np.log(sigma)
    h = lam[1:] - lam[:-1]
    rows = {k: np.zeros(n) for k in "abcdpq"}
    rows["hist"], rows["noise"] = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for k in range(n):
        if parametrization == "predict_noise":
            p, q = 1.0 / alpha[k], -sigma[k] / alpha[k]
        else:
            p, q = 0.0, 1.0
        second = order == 2 and k > 0 and not (lower_order_final and k == n - 1)
        if second:
            r = h[k - 1] / h[k]
            w0, w1 = 1.0 + 1.0 / (2.0 * r), -1.0 / (2.0 * r)
        else:
            w0, w1 = 1.0, 0.0
        if kind == "dpmsolver++":
            A, phi, c = sigma[k + 1] / sigma[k], alpha[k + 1] * -np.expm1(-h[k]), 0.0
        else:
            A, phi = sigma[k + 1] / sigma[k] * np.exp(-h[k]), alpha[k + 1] * -np.expm1(-2.0 * h[k])
            c = sigma[k + 1] * np.sqrt(-np.expm1(-2.0 * h[k]))
        rows["a"][k], rows["b"][k], rows["c"][k], rows["d"][k] = A + phi * w0 * p, phi * w0 * q, c, phi * w1
        if unfolded:
            rows["a"][k], rows["b"][k] = A, phi * w0
        rows["p"][k], rows["q"][k] = p, q
        rows["hist"][k] = int(w1 != 0.0)
        rows["noise"][k] = int(kind == "sde-dpmsolver++")
    return rows


def multistep_grid(n_steps, t0=999):
    """The integer timestep grid of an N-evaluation DPM-Solver++ run: N + 1 points from t0 (999; lower: an image-to-image start) down
    to 0; the model sees the first N."""
    n = int(n_steps)
    if not 1 <= n <= 999:
        raise ValueError(f"DPM-Solver++ steps must be in [1, 999], not {n}")
    if n > t0:
        raise ValueError(f"{n} DPM-Solver++ steps do not fit a start at t = {t0}: lower the steps or raise the strength")
    return np.linspace(t0, 0, n + 1).round().astype(int)


def _data_prediction(parametrization, ab_t):
    """(p, q) of x0 = p x + q m in float64 at alphas_bar ab_t: the model predicts the noise or the data"""
    if parametrization == "predict_previous":
        raise ValueError("x0 thresholding needs a model that predicts the noise or the data (predict_noise / predict_original), "
                         "not predict_previous: there is no x0")
    if parametrization == "predict_original":
        return 0.0, 1.0
    if parametrization != "predict_noise":
        raise ValueError(parametrization)
    return 1.0 / np.sqrt(ab_t), -np.sqrt(1.0 - ab_t) / np.sqrt(ab_t)


def unfolded_rows(kind, ts, eta=0.0, parametrization="predict_noise"):
    """The reference's own samplers as float64 UNFOLDED rows of the thresholded loop (x' = a x + b xh + c z, xh the thresholded
    x0 = p x + q m, no history), from the engine's bit-exact tables:
      "ddim"  over the descending grid ts (N + 1 timesteps), step t -> s: a = dir / sigma_t, b = alpha_s - a alpha_t with
              dir = sqrt(1 - abar_s - sig2), sig2 = betas_tilde[t] eta and c = sig2 (the reference scales its noise by sigma^2,
              sampler.py:112-120, and reads the model output as the noise whatever the parametrization: so does (p, q) here)
      "ddpm"  the ancestral steps at the timesteps ts (t -> t - 1): the posterior mean's coefficients on x and x0 (sampler.py:59-72)
              and c = sqrt(betas_tilde[t]); (p, q) from the parametrization
    Returns a dict of float64 arrays a, b, c, d, p, q and int32 arrays hist (0), noise (the step does not land on the final image)."""
    tb = {k: v.astype(np.float64) for k, v in schedule_tables().items()}
    ab = tb["alphas_bar"]
    ts = np.asarray(ts, np.int64)
    if kind == "ddim":
        t, s_ = ts[:-1], ts[1:]
        sig2 = tb["betas_tilde"][t] * float(eta)
        with np.errstate(invalid="ignore"):     # (a large eta on the step onto t = 0: the reference's direction term is NaN, sampler.py:116)
            a = np.sqrt(1.0 - ab[s_] - sig2) / np.sqrt(1.0 - ab[t])
        b = np.sqrt(ab[s_]) - a * np.sqrt(ab[t])
        c, noise = sig2, s_ > 0
        pq = [_data_prediction("predict_noise", v) for v in ab[t]]
        if parametrization == "predict_previous":
            _data_prediction(parametrization, 0.5)
    elif kind == "ddpm":
        t = ts
        a = np.sqrt(tb["alphas"][t]) * (1.0 - tb["alphas_bar_previous"][t]) / (1.0 - ab[t])
        b = np.sqrt(tb["alphas_bar_previous"][t]) * tb["betas"][t] / (1.0 - ab[t])
        c, noise = np.sqrt(tb["betas_tilde"][t]), t > 0
        pq = [_data_prediction(parametrization, v) for v in ab[t]]
    else:
        raise ValueError(kind)
    n = len(t)
    return {"a": a, "b": b, "c": np.asarray(c, np.float64), "d": np.zeros(n), "p": np.array([v[0] for v in pq]).reshape(n),
            "q": np.array([v[1] for v in pq]).reshape(n), "hist": np.zeros(n, np.int32), "noise": noise.astype(np.int32)}


def unfolded_coefficients(kind, ts, eta=0.0, parametrization="predict_noise"):
    """unfolded_rows as the fp32 rows a loop takes (each coefficient rounded once), with t: the model timesteps"""
    ts = np.asarray(ts, np.int64)
    r = unfolded_rows(kind, ts, eta, parametrization)
    out = {k: r[k].astype(np.float32) for k in "abcdpq"}
    out["t"] = (ts[:-1] if kind == "ddim" else ts).astype(np.float32)
    out["hist"], out["noise"] = r["hist"], r["noise"]
    return out


def multistep_coefficients(kind, ts, order=2, parametrization="predict_noise", unfolded=False):
    """The fp32 rows of a DPM-Solver++ run over the integer grid ts (descending, N + 1 timesteps, the last one usually 0), from the
    engine's bit-exact schedule tables: multistep_rows in float64, each coefficient rounded once.  Returns a dict of per-step arrays
    t (float32 model timesteps t_0 .. t_{N-1}), a, b, c, d, p, q (float32), hist, noise (int32).  The SDE draws z on every step but
    one landing on t = 0 (the reference's DDPM / DDIM convention)."""
    ts = np.asarray(ts, np.int64)
    if ts.ndim != 1 or len(ts) < 2 or (ts < 0).any() or (ts > 999).any() or (np.diff(ts) >= 0).any():
        raise ValueError("ts must be a strictly decreasing grid of timesteps in [0, 999] with at least two points")
    ab = schedule_tables()["alphas_bar"].astype(np.float64)[ts]
    r = multistep_rows(kind, ab, order, parametrization, unfolded=unfolded)
    out = {k: r[k].astype(np.float32) for k in "abcdpq"}
    out["t"] = ts[:-1].astype(np.float32)
    out["hist"] = r["hist"]
    out["noise"] = (r["noise"] * (ts[1:] > 0)).astype(np.int32)
    return out


class StepPlan(NamedTuple):
    """What get_samples runs, step by step.  kind: "ddpm" (dd_sample / ddpm_step: the update follows from t), "affine" (rows a, b, c)
    or "multistep" (rows a, b, c, d, p, q, hist: multistep_coefficients).  rows: per-step arrays, always with t (the model timestep,
    float32) and noise (int32: the step draws z).  save_after[k]: x is saved after step k.  switch_after: the first step the late model
    runs, or None; it may lie past the last step (a DDPM switch beyond num_steps), where it only hands the late model to dd_sample.
    lands[k]: the timestep whose noise level x has after step k, -1 for the final image (known_rows).
    moves: the walk of a plan with resampling jumps (walk_moves; empty: none).  Such a plan is of kind "affine", has one row per move
    and two more int32 rows, jump (1: the row is a jump, x' = a x + c z3, no model) and late (1: the step runs the late model);
    its switch_after is None.
    A plan with block caching (step_plan(..., cache_blocks= ...), cache_rows) is of kind "affine" and has two more rows, cache (int32: 0 the
    step refreshes its model's cache, 1 it reuses it, 2 it reuses an extrapolation of it) and cw (float32: the extrapolation weight)."""
    kind: str
    rows: dict
    save_after: list
    switch_after: Optional[int]
    lands: tuple = ()
    moves: tuple = ()


def start_timestep(strength=None):
    """The timestep a loop starts at: 999, or round(999 * strength) for an image-to-image start of strength in (0, 1]."""
    if strength is None:
        return 999
    if not (isinstance(strength, (int, float, np.number)) and 0 < float(strength) <= 1):
        raise ValueError(f"strength must be in (0, 1], not {strength!r}")
    return int(round(999 * float(strength)))


def walk_moves(n_steps, jumps):
    """The walk over a grid of positions p = 0 .. N (x at p < N carries the noise level of the timestep the model sees at step p,
    position N is the final image).  A step ("S", p) moves p -> p + 1 and evaluates the model at grid step p; a jump ("J", p, p - j)
    moves p -> p - j and runs no model.  jumps: {position: (length, count)}.  The walk steps from p = 0; after a step arrives at a
    position p < N that still has budget it spends one and jumps; budgets never refill.  A jump is legal only from 1 <= p < N with
    p - j >= 0 (never from the final image).  Returns the list of moves."""
    n = int(n_steps)
    if n < 1:
        raise ValueError("a walk needs at least one grid step")
    budget = {}
    for p, (length, count) in dict(jumps).items():
        p, length, count = int(p), int(length), int(count)
        if not 1 <= p < n or length < 1 or p - length < 0:
            raise ValueError(f"a jump of length {length} from position {p} is not legal on a grid of {n} steps")
        if count < 0:
            raise ValueError(f"jump count {count} at position {p} is negative")
        budget[p] = [length, count]
    moves, p = [], 0
    while p < n:
        moves.append(("S", p))
        p += 1
        if p < n and p in budget and budget[p][1] > 0:
            budget[p][1] -= 1
            moves.append(("J", p, p - budget[p][0]))
            p -= budget[p][0]
    return moves


def repaint_jumps(n_steps, jump, count):
    """RePaint's schedule (Lugmayr et al., 2022; get_schedule_jump of its code) with jump length j and r resamplings as walk_moves'
    jumps: the positions p with q = N - p >= 1, (q - 1) % j == 0 and p - j >= 0 get (j, r - 1)."""
    n, j, r = int(n_steps), int(jump), int(count)
    if j < 1:
        raise ValueError(f"resample_jump must be at least 1, not {jump}")
    if r < 1:
        raise ValueError(f"resample_count must be at least 1, not {count}")
    return {p: (j, r - 1) for p in range(1, n) if (n - p - 1) % j == 0 and p - j >= 0}


def restart_jumps(levels, restart):
    """Restart sampling (Xu et al., 2023) as walk_moves' jumps.  levels: the timestep the model sees at every grid position
    (descending); restart: (t_min, t_max, K) triples.  An interval snaps to the grid: lo = the position of the smallest level >= t_min,
    hi = the position of the largest level <= t_max, and lo gets (lo - hi, K): the walk comes down to lo, jumps back up to hi and
    repeats K times.  An interval that snaps to lo <= hi, or two that overlap on the grid, are ValueErrors."""
    levels = np.asarray(levels, np.float64)
    jumps, taken = {}, []
    for item in restart:
        try:
            t_min, t_max, k = item
            t_min, t_max, k = float(t_min), float(t_max), int(k)
        except (TypeError, ValueError):
            raise ValueError(f"a restart interval is (t_min, t_max, K), not {item!r}") from None
        if k < 1:
            raise ValueError(f"restart count K must be at least 1, not {k}")
        if not t_min < t_max:
            raise ValueError(f"restart interval needs t_min < t_max, not ({t_min:g}, {t_max:g})")
        above, below = np.nonzero(levels >= t_min)[0], np.nonzero(levels <= t_max)[0]
        if not len(above) or not len(below) or above[-1] <= below[0]:
            raise ValueError(f"restart interval ({t_min:g}, {t_max:g}) holds fewer than two levels of the grid")
        lo, hi = int(above[-1]), int(below[0])
        if any(hi < b and a < lo for a, b in taken):                           # (two intervals may share one grid point)
            raise ValueError(f"restart interval ({t_min:g}, {t_max:g}) overlaps another one on the grid")
        taken.append((hi, lo))
        jumps[lo] = (lo - hi, k)
    return jumps


def jump_coefficients(s, u):
    """(ja, jc) of the forward-noising jump from the noise level of timestep s up to that of timestep u >= s:
    x_u = ja x_s + jc z3 with ja = sqrt(abar[u] / abar[s]), jc = sqrt(1 - abar[u] / abar[s]), in float64 from the engine's tables,
    each rounded once."""
    ab = schedule_tables()["alphas_bar"].astype(np.float64)
    ratio = ab[int(u)] / ab[int(s)]
    return _f32(np.sqrt(ratio)), _f32(np.sqrt(1.0 - ratio))


def _walk_plan(base, parametrization, moves, timesteps_save):
    """The plan of a walk over the jump-free plan `base` (kind "affine", or the predict_noise "ddpm" plan, which becomes affine rows):
    a step row is base's row at the grid position, once per visit, a jump row is (a, b, c, noise) = (ja, 0, jc, 1) with the Philox
    counter of its own index like any row.  late[k]: what base runs at that position (the late model's rule stays by timestep);
    lands[k] of a jump: the level it reaches; save_after[k]: the last visit of a saved timestep."""
    if base.kind == "ddpm":
        ts = [int(t) for t in base.rows["t"]]
        grid = _affine_rows(ts, [affine_coefficients(parametrization, t) for t in ts], list(base.rows["noise"]))
    else:
        grid = base.rows
    level = [int(t) for t in grid["t"]]
    n = len(level)
    rows = {k: [] for k in ("t", "a", "b", "c", "noise", "jump", "late")}
    lands = []
    for mv in moves:
        if mv[0] == "S":
            p = mv[1]
            vals = (grid["t"][p], grid["a"][p], grid["b"][p], grid["c"][p], grid["noise"][p], 0,
                    int(base.switch_after is not None and p >= base.switch_after))
            lands.append(base.lands[p])
        else:
            _, p, u = mv
            ja, jc = jump_coefficients(level[p], level[u])
            vals = (grid["t"][u], ja, 0.0, jc, 1, 1, 0)
            lands.append(level[u])
        for k, v in zip(rows, vals):
            rows[k].append(v)
    rows = {k: np.array(v, np.int32 if k in ("noise", "jump", "late") else np.float32) for k, v in rows.items()}
    saves = set(int(v) for v in timesteps_save)
    last = {}
    for k, mv in enumerate(moves):
        if mv[0] == "S" and (1000 - level[mv[1]]) in saves:
            last[mv[1]] = k
    save_after = [False] * len(moves)
    for k in last.values():
        save_after[k] = True
    assert n == len(base.lands)
    return StepPlan("affine", rows, save_after, None, tuple(lands), tuple(moves))


def cache_settings(cache_blocks, cache_interval=3, cache_order=0, depths=()):
    """The checks of block caching's three numbers, before any model is built: K = cache_blocks >= 1 (and at most depth // 2 of every
    depth given), the refresh interval N >= 1, the order 0 or 1.  Returns (K, N, order) as ints."""
    try:
        k, n, order = int(cache_blocks), int(cache_interval), int(cache_order)
    except (TypeError, ValueError):
        raise ValueError(f"block caching takes integers (blocks, interval, order), not {(cache_blocks, cache_interval, cache_order)!r}") from None
    if k < 1:
        raise ValueError(f"cache_blocks must be at least 1, not {k}")
    if n < 1:
        raise ValueError(f"cache_interval must be at least 1, not {n}")
    if order not in (0, 1):
        raise ValueError(f"cache_order must be 0 or 1, not {order}")
    for depth in depths:
        if k > int(depth) // 2:
            raise ValueError(f"cache_blocks = {k} exceeds depth // 2 = {int(depth) // 2} of a model of depth {int(depth)}")
    return k, n, order


def cache_rows(t, switch_after, interval, order):
    """The block-caching rows of a plan whose steps see the model timesteps t, the late model from step switch_after on (None: never).
    Per model, j counts its steps from its first one (the late model starts again at 0 at the switch); step j refreshes iff
    j % interval == 0.  cache[k]: 0 a refresh, 1 a reuse, 2 (order 1) a reuse with extrapolation, where its model has refreshed twice:
    cw[k] = (t_1 - t_k) / (t_0 - t_1) with t_1 the last refresh's timestep and t_0 the one before it, in float64, rounded once.  A
    reuse step in front of a model's second refresh is a 1 under either order.  Returns (cache int32, cw float32)."""
    t = np.asarray(t, np.float64)
    n = len(t)
    cache, cw = np.zeros(n, np.int32), np.zeros(n, np.float32)
    first = 0
    t0 = t1 = None
    for k in range(n):
        if switch_after is not None and k == switch_after:
            first, t0, t1 = k, None, None
        if (k - first) % interval == 0:
            t0, t1 = t1, t[k]
        elif order == 1 and t0 is not None:
            cache[k], cw[k] = 2, np.float32((t1 - t[k]) / (t0 - t1))
        else:
            cache[k] = 1
    return cache, cw


def step_plan(parametrization, timesteps_save=(), has_late=False, t_switch=np.inf, num_steps=1000, use_ddim=False, ddim_steps=50,
              ddim_eta=0.0, solver=None, solver_steps=20, solver_order=2, strength=None, threshold=None, resample_jump=None,
              resample_count=None, restart=None, cache_blocks=None, cache_interval=3, cache_order=0):
    """The StepPlan of get_samples' arguments (parametrization: "predict_noise" | "predict_original" | "predict_previous", or None
    for a postprocessing function of elsewhere; has_late: a late model is given).  Host arithmetic only, no torch.
    strength (None or 1: the start at t = 999): the loops start at t0 = start_timestep(strength) -- DDPM at t0, the DDIM and solver grids
    built from t0 down with the same spacing rule and step count; the late model's rule is unchanged (by timestep).
    threshold (anything but None): the plan of the thresholded loop -- kind "multistep" on UNFOLDED rows for all three samplers
    (multistep_coefficients(..., unfolded=True), unfolded_coefficients); predict_previous has no x0 and is rejected.
    resample_jump = j with resample_count = r (RePaint's schedule, repaint_jumps) or restart = [(t_min, t_max, K), ...] (Restart
    sampling, restart_jumps): the plan of a walk over the grid of the plan without them (walk_moves, _walk_plan) -- kind "affine" for
    DDPM and DDIM alike.  Not with DPM-Solver++ (its history would have to restart behind a jump) or x0 thresholding, and not both
    at once; r == 1, or a j too long for any jump, gives the plan without them.
    cache_blocks = K (None: no caching) with cache_interval = N and cache_order: the plan with block caching -- kind "affine" for DDPM
    (predict_noise takes the affine rows a walk plan takes, so an N = 1 run is not promised bit-equal to the "ddpm"-kind loop) and DDIM,
    with the rows of cache_rows.  Not with DPM-Solver++, x0 thresholding, resampling jumps or parametrization None."""
    walk = resample_jump is not None or resample_count is not None or bool(restart)
    if cache_blocks is not None:
        _, interval, order = cache_settings(cache_blocks, cache_interval, cache_order)
        if solver is not None:
            raise ValueError("block caching is not supported with DPM-Solver++")
        if threshold is not None:
            raise ValueError("block caching is not supported with x0 thresholding")
        if walk:
            raise ValueError("block caching is not supported with resampling jumps")
        if parametrization is None:
            raise ValueError("block caching needs one of this module's predict_*_postprocessing functions")
        base = step_plan(parametrization, timesteps_save, has_late, t_switch, num_steps, use_ddim, ddim_steps, ddim_eta, strength=strength)
        rows = dict(base.rows)
        if base.kind == "ddpm":
            ts = [int(t) for t in rows["t"]]
            rows = _affine_rows(ts, [affine_coefficients(parametrization, t) for t in ts], list(rows["noise"]))
        rows["cache"], rows["cw"] = cache_rows(rows["t"], base.switch_after, interval, order)
        return base._replace(kind="affine", rows=rows)
    if walk:
        if (resample_jump is None) != (resample_count is None):
            raise ValueError("resample_jump and resample_count go together")
        if resample_jump is not None and restart:
            raise ValueError("RePaint's resampling (resample_jump / resample_count) and Restart sampling (restart) are exclusive")
        if solver is not None:
            raise ValueError("resampling jumps are not supported with DPM-Solver++: its history would have to restart behind a jump")
        if threshold is not None:
            raise ValueError("resampling jumps are not supported with x0 thresholding")
        base = step_plan(parametrization, timesteps_save, has_late, t_switch, num_steps, use_ddim, ddim_steps, ddim_eta, strength=strength)
        n = len(base.rows["t"])
        jumps = repaint_jumps(n, resample_jump, resample_count) if resample_jump is not None else restart_jumps(base.rows["t"], restart)
        moves = walk_moves(n, jumps)
        if len(moves) == n:
            return base
        return _walk_plan(base, parametrization, moves, timesteps_save)
    t0 = start_timestep(strength)
    if threshold is not None:
        _data_prediction(parametrization if parametrization is not None else "predict_noise", 0.5)
    # the DDPM loop switches AFTER the step at t == 1000 - t_switch (sampler.py:135-136): a t_switch outside [1, 1000] (0, negative,
    # > 1000, inf) never matches a t in 999..0, i.e. the first model runs every step
    in_range = has_late and np.isfinite(t_switch) and 1 <= int(t_switch) <= 1000
    if solver is not None:
        if use_ddim:
            raise ValueError("DPM-Solver++ and DDIM are exclusive")
        grid = multistep_grid(solver_steps, t0)                               # range check first
        if parametrization is None:
            raise ValueError("postprocessing must be one of this module's predict_*_postprocessing functions")
        kind, rows = "multistep", multistep_coefficients(solver, grid, solver_order, parametrization, unfolded=threshold is not None)
        switch_after = next((k for k, t in enumerate(rows["t"]) if t < 1000 - int(t_switch)), None) if in_range else None
        lands = [int(s) if s > 0 else -1 for s in grid[1:]]
    elif use_ddim:
        # reference sampler.py:103-126; z is drawn (:119) whenever s > 0, also at eta = 0
        ts = np.linspace(0, t0, ddim_steps).astype(int)[::-1]
        if (np.diff(ts) >= 0).any():
            raise ValueError(f"{ddim_steps} DDIM steps do not fit a start at t = {t0}: lower the steps or raise the strength")
        pairs = [(int(t), int(s)) for t, s in zip(ts[:-1], ts[1:])]
        if threshold is not None:
            if parametrization is None:
                raise ValueError("postprocessing must be one of this module's predict_*_postprocessing functions")
            kind, rows = "multistep", unfolded_coefficients("ddim", ts, ddim_eta, parametrization)
        else:
            kind, rows = "affine", _affine_rows([t for t, _ in pairs], [affine_coefficients("ddim", t, s, ddim_eta) for t, s in pairs],
                                                [s > 0 for _, s in pairs])
        # :122-123: the late model from the step after the first t < 1000 - t_switch (raw t_switch: <= 0 switches after step 0)
        switch_after = next((k + 1 for k, (t, _) in enumerate(pairs) if t < 1000 - t_switch), None) if has_late else None
        lands = [s if s > 0 else -1 for _, s in pairs]
    else:
        # sampler.py:129-139: t = 999 .. 1000 - num_steps; predict_original / predict_previous (:59-79) as affine rows
        ts = list(range(t0, max(t0 - int(num_steps), -1), -1))
        if threshold is not None and parametrization in ("predict_noise", "predict_original"):
            kind, rows = "multistep", unfolded_coefficients("ddpm", ts, 0.0, parametrization)
        elif parametrization == "predict_noise":
            kind, rows = "ddpm", {"t": np.array(ts, np.float32), "noise": np.array([t > 0 for t in ts], np.int32)}
        elif parametrization in ("predict_original", "predict_previous"):
            kind, rows = "affine", _affine_rows(ts, [affine_coefficients(parametrization, t) for t in ts], [t > 0 for t in ts])
        else:
            raise ValueError("postprocessing must be one of this module's predict_*_postprocessing functions")
        switch_after = max(int(t_switch) - (999 - t0), 0) if in_range else None   # the step after t == 1000 - t_switch
        lands = [t - 1 for t in ts]
    saves = set(int(v) for v in timesteps_save)
    return StepPlan(kind, rows, [(1000 - int(t)) in saves for t in rows["t"]], switch_after, tuple(lands))


def known_rows(plan):
    """The known-region rows (ka, kb) of a plan, float32, one per step: a step that lands on timestep s puts its known pixels at
    ka x0 + kb z2 with ka = sqrt(alphas_bar[s]), kb = sqrt(1 - alphas_bar[s]) from the engine's bit-exact tables, each rounded once;
    a step that lands on the final image (the DDPM step at t = 0, the last DDIM pair, the solver grid's last point) has (1, 0), so the
    known pixels of the result are x0 itself.  Host arithmetic only."""
    ab = schedule_tables()["alphas_bar"].astype(np.float64)
    s = np.asarray(plan.lands, np.int64)
    final = s < 0
    abs_ = ab[np.where(final, 0, s)]
    ka = np.where(final, 1.0, np.sqrt(abs_)).astype(np.float32)
    kb = np.where(final, 0.0, np.sqrt(1.0 - abs_)).astype(np.float32)
    return ka, kb


SCAN_PARAMETRIZATIONS = ("predict_noise", "predict_original", "predict_previous")


def scan_rows(timesteps, parametrization):
    """The fp32 rows of the denoising-error scan (dd_scan_error) at the integer timesteps given, from the engine's bit-exact schedule
    tables, each coefficient computed in float64 and rounded once:
        x_t = ka x0 + kb z with ka = sqrt(alphas_bar[t]), kb = sqrt(1 - alphas_bar[t])  -- what known_rows gives a step landing on t
        tgt = tz z + t0 x0 + tx x_t, the training target of the reference (trainer.py:319-352): predict_noise (1, 0, 0), predict_original
        (0, 1, 0), predict_previous (0, clean_image_coef, noisy_image_coef) = (0, sqrt(abar_prev) beta / (1 - abar), sqrt(alpha) (1 - abar_prev) / (1 - abar))
    Returns a dict of float32 arrays t, ka, kb, tz, t0, tx.  Host arithmetic only."""
    if parametrization not in SCAN_PARAMETRIZATIONS:
        raise ValueError(f"parametrization must be one of {SCAN_PARAMETRIZATIONS}, not {parametrization!r}")
    ts = np.asarray(timesteps, np.int64)
    if ts.ndim != 1 or len(ts) < 1 or (ts < 0).any() or (ts > 999).any():
        raise ValueError("timesteps must be a non-empty list of integers in [0, 999]")
    tb = {k: v.astype(np.float64) for k, v in schedule_tables().items()}
    ab = tb["alphas_bar"][ts]
    n = len(ts)
    if parametrization == "predict_noise":
        tz, t0, tx = np.ones(n), np.zeros(n), np.zeros(n)
    elif parametrization == "predict_original":
        tz, t0, tx = np.zeros(n), np.ones(n), np.zeros(n)
    else:
        ab_p = tb["alphas_bar_previous"][ts]
        tz = np.zeros(n)
        t0 = np.sqrt(ab_p) * tb["betas"][ts] / (1.0 - ab)
        tx = np.sqrt(tb["alphas"][ts]) * (1.0 - ab_p) / (1.0 - ab)
    rows = {"t": ts, "ka": np.sqrt(ab), "kb": np.sqrt(1.0 - ab), "tz": tz, "t0": t0, "tx": tx}
    return {k: np.ascontiguousarray(v, np.float32) for k, v in rows.items()}


def _affine_rows(ts, coefficients, noise):
    a, b, c = zip(*coefficients) if coefficients else ((), (), ())
    return {"t": np.array(ts, np.float32), "a": np.array(a, np.float32), "b": np.array(b, np.float32), "c": np.array(c, np.float32),
            "noise": np.array(noise, np.int32)}


def _segments(save_after):
    """(k0, k1) of the device loop cut after every save step"""
    k0 = 0
    for k, save in enumerate(save_after):
        if save or k == len(save_after) - 1:
            yield k0, k + 1
            k0 = k + 1
