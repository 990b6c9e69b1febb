"""get_samples' host logic without a GPU: the step plan (sampler.step_plan) and the engine calls get_samples makes from it.

The plan tests pin each sampler's rules: timesteps, update rows, which steps draw z, the save points and the step the late model
takes over.  The call-log tests run get_samples on the CPU with recording fakes for the models, the context, the autoencoder and the
device loops, and compare every call with a log recorded from the sampler as it was before get_samples was last restructured
(tests/golden/sampler_calls.json.gz): the matrix of samplers, noise modes, saves, switches, labels and classifier-free guidance, and
on top of it known regions, init images, x0 thresholds, autoguidance, perturbed-attention guidance and per-image seeds.  Floats are
logged as float32 bit patterns and tensors as their exact float64 sums, so the logs pin the coefficient rounding and the order of the
torch CPU noise draws.  A loop call without a late model drops switch_after / t_switch from its log: the engine ignores them there.
Every option get_samples rejects is rejected before the first call.

Regenerate the fixture (only when the intended behaviour changes): python tests/test_sampling_plan.py --write
"""
import contextlib
import gzip
import inspect
import json
import math
import sys
import types
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
    if isinstance(v, tuple) and hasattr(v, "_fields"):      # KnownRegion, Autoguidance, Perturbed, X0Threshold: by member
        return [type(v).__name__, {k: _norm(getattr(v, k)) for k in v._fields}]
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
    """ddpm_step / affine_step / multistep_step / threshold_step / known_blend / to_images: logged, and each adds 1 to x so the log
    tracks x's state; noise_images: image i filled with its seed; image_seeds: enter and exit logged around the calls inside"""

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

    def threshold_step(self, x, m, z, h, threshold, a, b, c, d, p, q, use_hist, out=None):
        self.log.add("threshold_h", h=h)
        h.add_(1)
        return self._step("threshold_step", x, out, m=m, z=z, threshold=threshold, a=a, b=b, c=c, d=d, p=p, q=q, use_hist=use_hist)

    def known_blend(self, x, x0, mask, z2, ka, kb, out=None):
        return self._step("known_blend", x, out, x0=x0, mask=mask, z2=z2, ka=ka, kb=kb)

    def noise_images(self, B, C, S, seed=0, image_seeds=None, counter=0):
        self.log.add("noise_images", B=B, C=C, S=S, seed=seed, image_seeds=image_seeds, counter=counter)
        return torch.stack([torch.full((C, S, S), float(s)) for s in image_seeds])

    @contextlib.contextmanager
    def image_seeds(self, seeds):
        self.log.add("image_seeds_enter", seeds=seeds)
        try:
            yield
        finally:
            self.log.add("image_seeds_exit", seeds=seeds)

    def to_images(self, x):
        self.log.add("to_images", x=x)
        return x.permute(0, 2, 3, 1) * 0.5 + 0.5


class _Model:
    """The UViT and its engine model in one: engine_model returns itself; forward writes t into out"""
    device = "cpu"
    depth = 3

    def __init__(self, name, log, ctx, num_classes=11):
        self.name, self.log, self.ctx, self.mp = name, log, ctx, types.SimpleNamespace(num_classes=num_classes)

    def engine_model(self, rows):
        self.log.add("engine_model", model=self, rows=rows)
        return self

    def forward(self, x, t, y=None, out=None):
        self.log.add("forward", model=self, x=x, t=t, y=y)
        return out.fill_(float(t))

    def forward_guided(self, x, t, y, scale, null_label, out=None):
        self.log.add("forward_guided", model=self, x=x, t=t, y=y, scale=scale, null_label=null_label)
        return out.fill_(float(t) + 0.5)

    def forward_autoguided(self, x, t, y, guide, scale, out=None):
        self.log.add("forward_autoguided", model=self, x=x, t=t, y=y, guide=guide, scale=scale)
        return out.fill_(float(t) + 0.25)

    def forward_perturbed(self, x, t, y, scale, layers, out=None):
        self.log.add("forward_perturbed", model=self, x=x, t=t, y=y, scale=scale, layers=layers)
        return out.fill_(float(t) + 0.75)

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
        if "t_start" in kw:
            kw["x"].add_(kw["t_start"] - kw["t_end"] + 1)
        elif "rows" not in kw:
            kw["x"].add_(len(kw["t"]))
        else:
            kw["x"].add_(len(kw["rows"]["t"]))
            kw["h"].add_(1)
        return kw["x"]
    return fake


LOOPS = (engine.sample_loop, engine.sample_affine_loop, engine.sample_multistep_loop, engine.sample_region_loop,
         engine.sample_affine_region_loop, engine.sample_multistep_region_loop, engine.sample_multistep_threshold_loop)


def record(monkeypatch, kw, log=None):
    """get_samples(**kw) with fakes: the call log, ending with the returned samples and intermediates"""
    log = _Log() if log is None else log
    ctx = _Ctx(log)
    for fn in LOOPS:
        monkeypatch.setattr(sampler, fn.__name__, _loop_fake(log, fn))
    kw = dict(kw)
    kw["model"] = _Model("first", log, ctx, kw.pop("first_classes", 11))
    if kw.pop("late", False):
        kw["late_model"] = _Model("late", log, ctx)
    if kw.pop("guide", False):
        kw["guide_model"] = _Model("guide", log, ctx)
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

    # ---- the options that came after the plan: each on a plain run and on one with saves and a late model that switches inside it
    def add(tag, names, extra, noises=("device", "torch_cpu"), runs=None):
        for name in names:
            kw, saves, switches = (runs or samplers)[name]
            for noise in noises:
                c = dict(base, **kw, noise=noise, **extra)
                out[f"{name}-{noise}-{tag}"] = c
                out[f"{name}-{noise}-{tag}-late{switches[0]}-saves"] = dict(c, late=True, t_switch=switches[0], timesteps_save=saves)

    # (a leading-1 image broadcast over the batch; a mask per image with 0, 1 and a fractional value)
    region = dict(known_image=np.linspace(-1, 1, 48, dtype=np.float32).reshape(1, 3, 4, 4),
                  known_mask=np.tile(np.float32([0, 1, 0.25, 1]), 8).reshape(2, 1, 4, 4))
    # strength 0.5 starts at t0 = 500.  DDPM t = 500 .. 489 (1000 - t = 500 .. 511, t_switch 504: the late model from step 5);
    # DDIM t = 500, 428, 357, 285, 214, 142, 71; the solver's grid 500, 417, 333, 250, 167, 83: t_switch 700 switches at the first t < 300
    init = dict(init_image=np.cos(np.arange(96, dtype=np.float32)).reshape(2, 3, 4, 4), strength=0.5)
    init_runs = {"ddpm": (samplers["ddpm"][0], [503, 507, 3], [504]), "ddim": (samplers["ddim"][0], [572, 715, 144], [700]),
                 "ode": (samplers["ode"][0], [583, 750, 2], [700])}
    static, dynamic = engine.X0Threshold("static", range=0.75), engine.X0Threshold("dynamic", quantile=0.9, s_max=2.5)
    add("known", ("ddpm", "original", "ddim", "ode"), region)
    add("init", ("ddpm", "ddim", "ode"), init, runs=init_runs)
    add("init-known", ("ddim",), dict(init, **region), runs=init_runs)
    add("clip", ("ddpm", "ddim", "ode"), dict(threshold=static))
    add("dynamic", ("ddpm", "ddim", "ode"), dict(threshold=dynamic))
    add("clip-known", ("ode",), dict(region, threshold=static))
    # autoguidance: the first model guides the late one (only the pair variant exists), an explicit guide, labels with an unconditional guide
    add("autoguided", ("ddpm", "ddim", "ode"), dict(autoguidance_scale=0.75, late=True))
    add("autoguided-explicit", ("ddpm", "ddim", "ode"), dict(autoguidance_scale=1.25, guide=True))
    add("autoguided-labels", ("ddpm", "ddim", "ode"), dict(autoguidance_scale=0.5, late=True, y=[4, 9], first_classes=0))
    # PAG: one model (no layers_late given / a bit mask), a pair (its saves leave a segment that starts on the late model)
    add("pag", ("ddpm", "ddim", "ode"), dict(pag=(1.5, [1])))
    add("pag-masks", ("ddpm",), dict(pag=(0.0, 0b101, 0b010), y=[4, 9]))
    add("pag-pair", ("ddpm", "ddim", "ode"), dict(pag=(1.5, [1], [0, 2]), late=True))
    add("image_seeds", ("ddpm", "ode"), dict(image_seeds=[7, 5], timesteps_save=[3, samplers["ode"][1][0]]), noises=("device",))
    add("image_seeds-labels-ae", ("ode",), dict(image_seeds=[2 ** 40, 0], y=[1, 2], ae=True), noises=("device",))
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


def _rejections():
    """name -> (arguments on top of ddim-device, the error's text): every ValueError get_samples raises itself, and a few inputs wrong
    in two ways, which raise the error the checks meet first"""
    img, mask = np.zeros((1, 3, 4, 4), np.float32), np.ones((1, 1, 4, 4), np.float32)
    clip = engine.X0Threshold("static")
    pag_with = "perturbed-attention guidance does not combine"
    return {
        "autoguidance+cfg": (dict(autoguidance_scale=1.0, cfg_scale=1.0, y=[1, 2], late=True), "autoguidance are exclusive"),
        "autoguidance-inf": (dict(autoguidance_scale=math.inf, late=True), "autoguidance_scale must be finite"),
        "autoguidance-nan": (dict(autoguidance_scale=math.nan, guide=True), "autoguidance_scale must be finite"),
        "autoguidance-no-guide": (dict(autoguidance_scale=1.0), "autoguidance needs a guide model"),
        "guide-no-scale": (dict(guide=True), "guide_model without autoguidance_scale"),
        "pag+cfg": (dict(pag=(1.0, [1]), cfg_scale=1.0, y=[1, 2]), pag_with),
        "pag+autoguidance": (dict(pag=(1.0, [1]), autoguidance_scale=1.0, late=True), pag_with),
        "pag+known": (dict(pag=(1.0, [1]), known_image=img, known_mask=mask), pag_with),
        "pag+init": (dict(pag=(1.0, [1]), init_image=img, strength=0.5), pag_with),
        "pag+threshold": (dict(pag=(1.0, [1]), threshold=clip), pag_with),
        "pag-inf": (dict(pag=(math.inf, [1])), "pag scale must be finite"),
        "pag-layer-first": (dict(pag=(1.0, [3])), "pag layers_first names a block at or above the model's depth 3"),
        "pag-layer-late": (dict(pag=(1.0, [1], 0b1000), late=True), "pag layers_late names a block at or above the model's depth 3"),
        "image_seeds-torch_cpu": (dict(image_seeds=[1, 2], noise="torch_cpu"), "image_seeds need noise='device'"),
        "image_seeds-length": (dict(image_seeds=[1, 2, 3]), "image_seeds holds 3 seeds for batch_size 2"),
        "init-no-strength": (dict(init_image=img), "init_image and strength go together"),
        "strength-no-init": (dict(strength=0.5), "init_image and strength go together"),
        "known-no-mask": (dict(known_image=img), "known_image and known_mask go together"),
        "mask-no-known": (dict(known_mask=mask), "known_image and known_mask go together"),
        "mask-above": (dict(known_image=img, known_mask=mask * 1.5), r"known_mask must lie in \[0, 1\]"),
        "mask-below": (dict(known_image=img, known_mask=mask - 1.5), r"known_mask must lie in \[0, 1\]"),
        "mask-shape": (dict(known_image=img, known_mask=np.ones((1, 3, 4, 4), np.float32)), "known_mask must have shape"),
        "threshold-ae": (dict(threshold=clip, ae=True), "x0 thresholding is for pixel-space models"),
        "threshold-previous": (dict(threshold=clip, post="predict_previous"), "x0 thresholding needs a model that predicts"),
        "threshold-mode": (dict(threshold=engine.X0Threshold("soft")), "threshold mode must be"),
        "cfg-no-labels": (dict(cfg_scale=1.0), "classifier-free guidance needs class labels"),
        # wrong in two ways: the first check met wins
        "noise, then autoguidance+cfg": (dict(noise="philox", autoguidance_scale=1.0, cfg_scale=1.0), "noise must be"),
        "autoguidance+cfg, then no guide": (dict(autoguidance_scale=math.inf, cfg_scale=1.0), "autoguidance are exclusive"),
        "guide-no-scale, then pag": (dict(guide=True, pag=(math.inf, [7])), "guide_model without autoguidance_scale"),
        "pag+cfg, then labels": (dict(pag=(math.inf, [7]), cfg_scale=1.0), pag_with),
        "pag-inf, then layer": (dict(pag=(math.inf, [7])), "pag scale must be finite"),
        "pag, then image_seeds": (dict(pag=(1.0, [3]), image_seeds=[1]), "pag layers_first"),
        "image_seeds, then init": (dict(image_seeds=[1], init_image=img), "image_seeds holds 1 seeds"),
        "init, then known": (dict(init_image=img, known_mask=mask), "init_image and strength go together"),
        "known, then plan": (dict(known_image=img, solver="dpmsolver++"), "known_image and known_mask go together"),
        "plan, then threshold-ae": (dict(threshold=clip, ae=True, post="predict_previous"), "x0 thresholding needs a model that predicts"),
        "threshold-ae, then labels": (dict(threshold=clip, ae=True, cfg_scale=1.0), "x0 thresholding is for pixel-space models"),
        "labels, then mask": (dict(cfg_scale=1.0, known_image=img, known_mask=mask * 2), "classifier-free guidance needs class labels"),
    }


REJECTIONS = _rejections()


@pytest.mark.parametrize("name", sorted(REJECTIONS))
def test_bad_options_raise_before_any_call(monkeypatch, name):
    extra, text = REJECTIONS[name]
    log = _Log()
    with pytest.raises(ValueError, match=text):
        record(monkeypatch, dict(CASES["ddim-device"], **extra), log)
    assert log == []


def test_image_seeds_need_square_images(monkeypatch):
    """(raised where x_T is drawn, behind the models' engine_model calls)"""
    with pytest.raises(ValueError, match="image_seeds: square images only"):
        record(monkeypatch, dict(CASES["ddpm-device"], image_seeds=[1, 2], sample_width=6))


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
