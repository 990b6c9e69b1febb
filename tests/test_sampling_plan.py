"""get_samples' host logic without a GPU: the step plan (sampler.step_plan) and the engine calls get_samples makes from it.

The plan tests pin each sampler's rules: timesteps, update rows, which steps draw z, the save points and the step the late model
takes over.  The call-log tests run get_samples on the CPU with recording fakes for the models, the context, the autoencoder and the
three device loops, and compare every call with a log recorded once from the sampler before the plan existed
(tests/golden/sampler_calls.json.gz).  Floats are logged as float32 bit patterns and tensors as their exact float64 sums, so the
logs pin the coefficient rounding and the order of the torch CPU noise draws.  A loop call without a late model drops switch_after /
t_switch from its log: the engine ignores them there.

Regenerate the fixture (only when the intended behaviour changes): python tests/test_sampling_plan.py --write
"""
import gzip
import inspect
import json
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from duodiff_amd import engine, sampler  # noqa: E402

FIXTURE = Path(__file__).resolve().parent / "golden" / "sampler_calls.json.gz"


def _bits(v):
    return np.asarray(v, np.float32).view(np.uint32).tolist()


# ---- the step plan ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t_switch,switch_after", [(300, 300), (1, 1), (1000, 1000), (300.7, 300), (0, None), (-3, None),
                                                   (1001, None), (math.inf, None)])
def test_plan_ddpm(t_switch, switch_after):
    """t = 999 .. 1000 - num_steps, z iff t > 0; the late model from the step after t == 1000 - t_switch, only for t_switch in [1, 1000],
    even past num_steps (dd_sample is then still handed the late model)"""
    p = sampler.step_plan("predict_noise", has_late=True, t_switch=t_switch)
    assert p.kind == "ddpm" and sorted(p.rows) == ["noise", "t"]
    assert p.rows["t"].tolist() == list(range(999, -1, -1)) and p.rows["noise"].tolist() == [1] * 999 + [0]
    assert p.switch_after == switch_after and p.save_after == [False] * 1000
    if switch_after is not None and switch_after < 1000:
        assert p.rows["t"][switch_after - 1] == 1000 - int(t_switch)
    assert sampler.step_plan("predict_noise", has_late=False, t_switch=t_switch).switch_after is None
    short = sampler.step_plan("predict_noise", has_late=True, t_switch=t_switch, num_steps=5)
    assert short.rows["t"].tolist() == [999, 998, 997, 996, 995] and short.switch_after == switch_after


@pytest.mark.parametrize("kind", ["predict_original", "predict_previous"])
def test_plan_parametrizations(kind):
    """the DDPM loop's steps, noise and switch with the rows affine_coefficients(kind, t), bit for bit"""
    p = sampler.step_plan(kind, [1, 4, 700], has_late=True, t_switch=3, num_steps=6)
    assert p.kind == "affine" and p.rows["t"].tolist() == [999, 998, 997, 996, 995, 994] and p.rows["noise"].tolist() == [1] * 6
    want = [sampler.affine_coefficients(kind, t) for t in range(999, 993, -1)]
    for i, key in enumerate("abc"):
        assert _bits(p.rows[key]) == _bits([w[i] for w in want]), key
    assert p.switch_after == 3 and p.save_after == [True, False, False, True, False, False]
    assert sampler.step_plan(kind, num_steps=1000).rows["noise"][-1] == 0


@pytest.mark.parametrize("t_switch,switch_after", [(300, 4), (144, 3), (0, 1), (-5, 1), (999, None), (math.inf, None)])
def test_plan_ddim(t_switch, switch_after):
    """pairs of linspace(0, 999, ddim_steps).astype(int)[::-1], rows affine_coefficients("ddim", t, s, eta); z iff s > 0 also at eta 0;
    the late model from the step after the first t < 1000 - t_switch with the raw t_switch; num_steps and parametrization ignored"""
    for eta in (0.0, 0.3):
        p = sampler.step_plan(None, [144], has_late=True, t_switch=t_switch, num_steps=3, use_ddim=True, ddim_steps=8, ddim_eta=eta)
        ts = [999, 856, 713, 570, 428, 285, 142, 0]
        assert p.kind == "affine" and p.rows["t"].tolist() == ts[:-1] and p.rows["noise"].tolist() == [1] * 6 + [0]
        want = [sampler.affine_coefficients("ddim", t, s, eta) for t, s in zip(ts[:-1], ts[1:])]
        for i, key in enumerate("abc"):
            assert _bits(p.rows[key]) == _bits([w[i] for w in want]), key
        assert p.switch_after == switch_after and p.save_after == [False, True] + [False] * 5


@pytest.mark.parametrize("t_switch,switch_after", [(300, "first"), (1, 1), (1000, None), (0, None), (math.inf, None)])
def test_plan_solver(t_switch, switch_after):
    """the rows of multistep_coefficients on multistep_grid(solver_steps); the late model from the first k with t_k < 1000 - t_switch,
    t_switch in [1, 1000]; num_steps ignored"""
    for solver, param, steps in (("dpmsolver++", "predict_noise", 20), ("sde-dpmsolver++", "predict_original", 7)):
        p = sampler.step_plan(param, has_late=True, t_switch=t_switch, num_steps=3, solver=solver, solver_steps=steps)
        want = sampler.multistep_coefficients(solver, sampler.multistep_grid(steps), 2, param)
        assert p.kind == "multistep" and sorted(p.rows) == sorted(want)
        for key in want:
            assert p.rows[key].dtype == want[key].dtype and p.rows[key].tobytes() == want[key].tobytes(), key
        if switch_after == "first":
            assert p.switch_after == min(k for k, t in enumerate(want["t"]) if t < 700)
        else:
            assert p.switch_after == switch_after


def test_plan_solver_one_step():
    p = sampler.step_plan("predict_noise", [1], has_late=True, t_switch=1, solver="dpmsolver++", solver_steps=1)
    assert p.rows["t"].tolist() == [999] and p.save_after == [True] and p.switch_after is None
    p = sampler.step_plan("predict_noise", has_late=True, t_switch=1, solver="sde-dpmsolver++", solver_steps=1)
    assert p.rows["noise"].tolist() == [0] and p.rows["hist"].tolist() == [0]


def test_plan_saves_and_cuts():
    """save_after[k] iff 1000 - t_k is in timesteps_save (values the loop never visits are ignored); the device loop is cut after every
    save step, and a switch on a save point starts the next segment"""
    p = sampler.step_plan("predict_noise", [3, 7, 12, 500, 0, -1], has_late=True, t_switch=7, num_steps=12)
    assert [k for k, s in enumerate(p.save_after) if s] == [2, 6, 11] and p.switch_after == 7
    assert list(sampler._segments(p.save_after)) == [(0, 3), (3, 7), (7, 12)]
    assert list(sampler._segments([False] * 4)) == [(0, 4)] and list(sampler._segments([True, False])) == [(0, 1), (1, 2)]
    assert list(sampler._segments([])) == []


def test_plan_rejects_bad_arguments():
    with pytest.raises(ValueError, match="postprocessing"):
        sampler.step_plan(None)
    with pytest.raises(ValueError, match="exclusive"):
        sampler.step_plan("predict_noise", use_ddim=True, solver="dpmsolver++")
    with pytest.raises(ValueError, match="predict_previous"):
        sampler.step_plan("predict_previous", solver="dpmsolver++")
    with pytest.raises(ValueError, match="steps"):
        sampler.step_plan("predict_noise", solver="dpmsolver++", solver_steps=0)


# ---- recording fakes ------------------------------------------------------------------------------------------------------------
def _norm(v):
    """A JSON value that identifies v: floats as float32 bit patterns, tensors as (shape, exact float64 sum)"""
    if v is None or isinstance(v, (bool, str)):
        return v
    if isinstance(v, np.bool_):
        return bool(v)
    if isinstance(v, torch.Tensor):
        return ["tensor", list(v.shape), math.fsum(v.detach().double().flatten().tolist())]
    if isinstance(v, (_Model, _Ctx)):
        return [type(v).__name__, getattr(v, "name", "")]
    if isinstance(v, dict):
        return {k: _norm(v[k]) for k in sorted(v)}
    if isinstance(v, (list, tuple, np.ndarray)):
        a = np.asarray(v)
        if a.dtype.kind == "f":
            return ["f32", a.astype(np.float32).view(np.uint32).tolist()]
        if a.dtype.kind in "iub":
            return ["int", a.astype(np.int64).tolist()]
        return [_norm(e) for e in v]
    if isinstance(v, (int, float, np.number)):
        return ["f32", int(np.float32(v).view(np.uint32))]
    raise TypeError(type(v))


class _Log(list):
    def add(self, name, **kw):
        self.append([name, {k: _norm(v) for k, v in sorted(kw.items())}])


class _Ctx:
    """ddpm_step / affine_step / multistep_step / to_images: logged, and each step adds 1 to x so the log tracks x's state"""

    def __init__(self, log):
        self.log = log

    def _step(self, name, x, out, **kw):
        self.log.add(name, x=x, **kw)
        out = torch.empty_like(x) if out is None else out
        out.copy_(x + 1)
        return out

    def ddpm_step(self, x, eps, z, t, out=None):
        return self._step("ddpm_step", x, out, eps=eps, z=z, t=t)

    def affine_step(self, x, m, z, a, b, c, out=None):
        return self._step("affine_step", x, out, m=m, z=z, a=a, b=b, c=c)

    def multistep_step(self, x, m, z, h, a, b, c, d, p, q, use_hist, out=None):
        self.log.add("multistep_h", h=h)
        h.add_(1)
        return self._step("multistep_step", x, out, m=m, z=z, a=a, b=b, c=c, d=d, p=p, q=q, use_hist=use_hist)

    def to_images(self, x):
        self.log.add("to_images", x=x)
        return x.permute(0, 2, 3, 1) * 0.5 + 0.5


class _Model:
    """The UViT and its engine model in one: engine_model returns itself; forward writes t into out"""
    device = "cpu"

    def __init__(self, name, log, ctx):
        self.name, self.log, self.ctx = name, log, ctx

    def engine_model(self, rows):
        self.log.add("engine_model", model=self, rows=rows)
        return self

    def forward(self, x, t, y=None, out=None):
        self.log.add("forward", model=self, x=x, t=t, y=y)
        return out.fill_(float(t))

    def forward_guided(self, x, t, y, scale, null_label, out=None):
        self.log.add("forward_guided", model=self, x=x, t=t, y=y, scale=scale, null_label=null_label)
        return out.fill_(float(t) + 0.5)

    def sample_step(self, x, t, y=None, z=None, noise="buffer"):
        self.log.add("sample_step", model=self, x=x, t=t, y=y, z=z, noise=noise)
        return x.add_(1)


class _Autoencoder:
    def __init__(self, log):
        self.log = log

    def decode(self, x):
        self.log.add("decode", x=x)
        return x * 2


def _loop_fake(log, fn):
    """A recording stand-in for an engine loop: arguments bound to fn's signature (defaults filled in), x advanced by its step count"""
    sig = inspect.signature(fn)

    def fake(*args, **kwargs):
        b = sig.bind(*args, **kwargs)
        b.apply_defaults()
        kw = dict(b.arguments)
        if kw["late"] is None:
            kw.pop("switch_after", None)
            kw.pop("t_switch", None)
        log.add(fn.__name__, **kw)
        if fn is engine.sample_loop:
            kw["x"].add_(kw["t_start"] - kw["t_end"] + 1)
        elif fn is engine.sample_affine_loop:
            kw["x"].add_(len(kw["t"]))
        else:
            kw["x"].add_(len(kw["rows"]["t"]))
            kw["h"].add_(1)
        return kw["x"]
    return fake


def record(monkeypatch, kw, log=None):
    """get_samples(**kw) with fakes: the call log, ending with the returned samples and intermediates"""
    log = _Log() if log is None else log
    ctx = _Ctx(log)
    for fn in (engine.sample_loop, engine.sample_affine_loop, engine.sample_multistep_loop):
        monkeypatch.setattr(sampler, fn.__name__, _loop_fake(log, fn))
    kw = dict(kw)
    kw["model"] = _Model("first", log, ctx)
    if kw.pop("late", False):
        kw["late_model"] = _Model("late", log, ctx)
    if kw.pop("ae", False):
        kw["autoencoder"] = _Autoencoder(log)
    kw["postprocessing"] = getattr(sampler, kw.pop("post", "predict_noise") + "_postprocessing")
    samples, inter = sampler.get_samples(**kw)
    log.add("result", samples=torch.from_numpy(samples), inter=[torch.from_numpy(v) for v in inter])
    return log


# ---- the matrix ------------------------------------------------------------------------------------------------------------------
def _cases():
    base = dict(batch_size=2, seed=3, num_channels=3, sample_height=4, sample_width=4)
    solver_t = [1000 - int(t) for t in sampler.multistep_grid(6)[:-1]]            # 1000 - t of the solver's 6 steps
    samplers = {
        # DDPM-like loops over t = 999 .. 988: 1000 - t = 1 .. 12; saves after 1000 - t = 3 and 7 (500 is never reached)
        "ddpm": (dict(post="predict_noise", num_steps=12), [3, 7, 500], [2, 5, 7, 12, 30, 0, 1001, math.inf]),
        "original": (dict(post="predict_original", num_steps=12), [3, 7, 500], [2, 5, 7, 30, math.inf]),
        "previous": (dict(post="predict_previous", num_steps=12), [3, 7, 500], [5, 7, 30]),
        # DDIM over 7 steps t = 999, 856, 713, 570, 428, 285, 142 (saves: 1000 - t = 144, 430; 3 is never reached)
        "ddim": (dict(use_ddim=True, ddim_steps=8, ddim_eta=0.5), [144, 430, 3], [300, 430, 144, 2000, 0, -5, math.inf]),
        "ddim_eta0": (dict(use_ddim=True, ddim_steps=8), [144], [300, math.inf]),
        "ode": (dict(solver="dpmsolver++", solver_steps=6), [solver_t[1], solver_t[3], 2], [300, solver_t[3], 1, 1000, math.inf]),
        "sde": (dict(solver="sde-dpmsolver++", solver_steps=6, post="predict_original"), [solver_t[2]], [300, solver_t[2], math.inf]),
        "ode_1": (dict(solver="dpmsolver++", solver_steps=1, solver_order=1), [1], [500]),
    }
    out = {}
    for name, (kw, saves, switches) in samplers.items():
        for noise in ("device", "torch_cpu"):
            c = dict(base, **kw, noise=noise)
            out[f"{name}-{noise}"] = c
            out[f"{name}-{noise}-saves"] = dict(c, timesteps_save=saves)
            out[f"{name}-{noise}-late_noswitch"] = dict(c, late=True)
            for ts in switches:
                out[f"{name}-{noise}-late{ts}-saves"] = dict(c, late=True, t_switch=ts, timesteps_save=saves)
            out[f"{name}-{noise}-guided-late{switches[0]}-saves"] = dict(c, late=True, t_switch=switches[0], timesteps_save=saves,
                                                                         y=[4, 9], cfg_scale=0.75, cfg_null_label=10)
            out[f"{name}-{noise}-labels-ae-saves"] = dict(c, y=[1, 2], ae=True, timesteps_save=saves)
            out[f"{name}-{noise}-nograph"] = dict(c, use_graph=False, seed=11)
    # the full 1000-step DDPM loop on the device, with a switch and saves (one dd_sample call per segment)
    out["ddpm-device-1000"] = dict(base, noise="device", late=True, t_switch=300, timesteps_save=[100, 300, 301, 1000])
    out["ddpm-device-1000-guided-ae"] = dict(base, noise="device", late=True, t_switch=999, timesteps_save=[999], y=[0, 1],
                                              cfg_scale=0.0, ae=True)
    return out


CASES = _cases()


def _jsonable(log):
    return json.loads(json.dumps(log))


@pytest.fixture(scope="module")
def expected():
    with gzip.open(FIXTURE, "rt") as f:
        return json.load(f)


def test_fixture_covers_the_matrix(expected):
    assert sorted(expected) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_call_log_matches_the_parent(monkeypatch, expected, name):
    got = _jsonable(record(monkeypatch, CASES[name]))
    want = expected[name]
    assert len(got) == len(want), (len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w)


@pytest.mark.parametrize("name", [n for n in sorted(CASES) if n.endswith("-device-late_noswitch")])
def test_unknown_noise_mode_raises_before_any_call(monkeypatch, name):
    log = _Log()
    with pytest.raises(ValueError, match="noise"):
        record(monkeypatch, dict(CASES[name], noise="philox"), log)
    assert log == []


if __name__ == "__main__" and "--write" in sys.argv:
    mp = pytest.MonkeyPatch()
    logs = {}
    try:
        for name, kw in CASES.items():
            logs[name] = _jsonable(record(mp, kw))
            mp.undo()
    finally:
        mp.undo()
    with gzip.GzipFile(FIXTURE, "wb", mtime=0) as f:
        f.write(json.dumps(logs, sort_keys=True, separators=(",", ":")).encode())
    print(f"wrote {FIXTURE}: {len(logs)} cases, {sum(len(v) for v in logs.values())} calls")
