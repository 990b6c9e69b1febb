"""Block caching (DeepCache, Ma et al. 2024; order 1: TaylorSeer), the host side: the plan rows `cache` and `cw` of step_plan, every
rejection before a model is built, the ctypes binding, and the elementwise gate of the kernel test checked against wrong results.  No GPU.

Also home of what tests/test_block_cache.py shares with this file: the float64 reference of cache_extrapolate_kernel and its bound."""
import ctypes as C

import numpy as np
import pytest

from conftest import REPO
from duodiff_amd import _lib as L
from duodiff_amd import step_plan as sp
from kernel_support import bf16, gate, ulp_bf16
from loop_support import cli_argv

CONFIGS = REPO / "configs"
CELEBA = CONFIGS / "uvit_celeba.yaml"
CELEBA_3 = CONFIGS / "uvit_celeba_3.yaml"


# ---- the kernel's reference (shared with the GPU tests) ------------------------------------------------------------------------
def extrapolate_ref(last, prev, w, prec):
    """float64 last + w (last - prev) of the stored operands and the bound of the kernel's result: half an ulp of the reference in the
    activation type (bf16 mode) + 2^-22 (|last| + |w| (|last| + |prev|)) -- three fp32 roundings, each at most 2^-24 of its magnitude"""
    l64, p64 = np.asarray(last, np.float64), np.asarray(prev, np.float64)
    ref = l64 + float(w) * (l64 - p64)
    tol = 2.0 ** -22 * (np.abs(l64) + abs(float(w)) * (np.abs(l64) + np.abs(p64)))
    if prec == "bf16":
        tol = tol + 0.5 * ulp_bf16(ref)
    return ref, tol


def extrapolate_operands(rows, D, sigma, prec, seed):
    """last and prev [rows, D] as values of the activation type: a slowly moving feature at `sigma`"""
    r = np.random.default_rng(seed)
    last = (sigma * r.standard_normal((rows, D))).astype(np.float32)
    prev = (last + 0.1 * sigma * r.standard_normal((rows, D))).astype(np.float32)
    return (bf16(last), bf16(prev)) if prec == "bf16" else (last, prev)


# ---- the plan rows -----------------------------------------------------------------------------------------------------------
def _want_rows(t, switch_after, N, order):
    """cache / cw from the definition, written out independently of cache_rows: float64, rounded once"""
    cache, cw = [], []
    for k in range(len(t)):
        late = switch_after is not None and k >= switch_after
        k_first = switch_after if late else 0
        j = k - k_first
        if j % N == 0:
            cache.append(0); cw.append(np.float32(0))
            continue
        refreshes = [i for i in range(k_first, k) if (i - k_first) % N == 0]
        if order == 1 and len(refreshes) >= 2:
            t1, t0 = float(t[refreshes[-1]]), float(t[refreshes[-2]])
            cache.append(2); cw.append(np.float32((t1 - float(t[k])) / (t0 - t1)))
        else:
            cache.append(1); cw.append(np.float32(0))
    return np.array(cache, np.int32), np.array(cw, np.float32)


PLANS = {
    "ddpm7": dict(parametrization="predict_noise", num_steps=7),
    "ddim10": dict(parametrization="predict_noise", use_ddim=True, ddim_steps=11),
    "pair_ddpm": dict(parametrization="predict_noise", num_steps=12, has_late=True, t_switch=5),
    "pair_ddim": dict(parametrization="predict_original", use_ddim=True, ddim_steps=13, has_late=True, t_switch=400),
    "strength": dict(parametrization="predict_noise", use_ddim=True, ddim_steps=9, strength=0.6),
    "strength_ddpm": dict(parametrization="predict_previous", num_steps=8, strength=0.5, timesteps_save=[503, 505]),
}


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("N", [1, 2, 3, 5])
@pytest.mark.parametrize("name", sorted(PLANS))
def test_plan_rows(name, N, order):
    kw = dict(PLANS[name], timesteps_save=PLANS[name].get("timesteps_save", [2, 5]))
    base = sp.step_plan(**kw)
    plan = sp.step_plan(**kw, cache_blocks=1, cache_interval=N, cache_order=order)
    n = len(base.rows["t"])
    assert plan.kind == "affine" and len(plan.rows["t"]) == n
    assert plan.rows["cache"].dtype == np.int32 and plan.rows["cw"].dtype == np.float32
    assert plan.rows["cache"].shape == plan.rows["cw"].shape == (n,)
    assert np.array_equal(plan.rows["t"], base.rows["t"]) and np.array_equal(plan.rows["noise"], base.rows["noise"])
    assert plan.save_after == base.save_after and plan.switch_after == base.switch_after and plan.lands == base.lands and not plan.moves
    assert all(np.array_equal(a, b) for a, b in zip(sp.known_rows(plan), sp.known_rows(base)))
    if base.kind == "affine":
        for key in "abc":
            assert np.array_equal(plan.rows[key], base.rows[key])
    else:          # predict_noise DDPM: the affine rows a walk plan takes
        for k, t in enumerate(base.rows["t"]):
            assert (plan.rows["a"][k], plan.rows["b"][k], plan.rows["c"][k]) == sp.affine_coefficients("predict_noise", int(t))
    sw = plan.switch_after if plan.switch_after is not None and plan.switch_after < n else None
    cache, cw = _want_rows(plan.rows["t"], sw, N, order)
    assert np.array_equal(plan.rows["cache"], cache), (plan.rows["cache"], cache)
    assert np.array_equal(plan.rows["cw"].view(np.uint32), cw.view(np.uint32))
    assert plan.rows["cache"][0] == 0
    if sw is not None:
        assert plan.rows["cache"][sw] == 0, "the late model's first step is a refresh"
    if N == 1:
        assert not plan.rows["cache"].any()
    if order == 0:
        assert plan.rows["cache"].max(initial=0) <= 1 and not plan.rows["cw"].any()


def test_plan_rows_by_hand():
    """DDPM, 7 steps, N = 3, order 1: t = 999 .. 993; refreshes at steps 0, 3, 6; steps 1, 2 come before a second refresh (op 1);
    steps 4, 5 extrapolate from t_0 = 999, t_1 = 996: w = (996 - 995) / 3, (996 - 994) / 3"""
    plan = sp.step_plan("predict_noise", num_steps=7, cache_blocks=2, cache_interval=3, cache_order=1)
    assert list(plan.rows["cache"]) == [0, 1, 1, 0, 2, 2, 0]
    assert list(plan.rows["cw"]) == [0, 0, 0, 0, np.float32(1 / 3), np.float32(2 / 3), 0]
    # a pair with the switch inside, on a reuse position of the first model: the late model starts with a refresh and counts from there
    plan = sp.step_plan("predict_noise", num_steps=9, has_late=True, t_switch=4, cache_blocks=1, cache_interval=3, cache_order=1)
    assert plan.switch_after == 4
    assert list(plan.rows["cache"]) == [0, 1, 1, 0, 0, 1, 1, 0, 2]
    assert plan.rows["cw"][8] == np.float32((992 - 991) / (995 - 992))
    # DDIM: uneven grid spacing enters w
    plan = sp.step_plan("predict_noise", use_ddim=True, ddim_steps=11, cache_blocks=1, cache_interval=2, cache_order=1)
    t = plan.rows["t"].astype(np.float64)
    assert list(plan.rows["cache"]) == [0, 1, 0, 2, 0, 2, 0, 2, 0, 2]
    assert plan.rows["cw"][3] == np.float32((t[2] - t[3]) / (t[0] - t[2]))


# ---- rejections ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,match", [
    (dict(cache_blocks=0), "cache_blocks"),
    (dict(cache_blocks=-1), "cache_blocks"),
    (dict(cache_blocks=1, cache_interval=0), "cache_interval"),
    (dict(cache_blocks=1, cache_order=2), "cache_order"),
    (dict(cache_blocks=1, cache_order=-1), "cache_order"),
    (dict(cache_blocks=1, solver="dpmsolver++"), "DPM-Solver"),
    (dict(cache_blocks=1, threshold=object()), "thresholding"),
    (dict(cache_blocks=1, resample_jump=2, resample_count=2), "resampling"),
    (dict(cache_blocks=1, restart=[(100.0, 500.0, 1)]), "resampling"),
])
def test_step_plan_rejects(kw, match):
    with pytest.raises(ValueError, match=match):
        sp.step_plan("predict_noise", num_steps=8, **kw)


def test_step_plan_rejects_a_foreign_postprocessing():
    with pytest.raises(ValueError, match="postprocessing"):
        sp.step_plan(None, num_steps=8, cache_blocks=1)


def test_cache_settings():
    assert sp.cache_settings(2, 3, 1, depths=[5, 13]) == (2, 3, 1)
    assert sp.cache_settings(6, depths=[13]) == (6, 3, 0)
    with pytest.raises(ValueError, match="depth"):
        sp.cache_settings(7, 3, 0, depths=[13])
    with pytest.raises(ValueError, match="depth"):
        sp.cache_settings(2, 3, 0, depths=[13, 3])          # either model's depth // 2
    with pytest.raises(ValueError, match="integers"):
        sp.cache_settings("two")


@pytest.mark.parametrize("extra,match", [
    (["--cache_blocks", "7"], "depth"),                                          # uvit_celeba: depth 13, depth // 2 = 6
    (["--cache_blocks", "0"], "cache_blocks"),
    (["--cache_blocks", "2", "--cache_interval", "0"], "cache_interval"),
    (["--cache_interval", "3"], "need --cache_blocks"),
    (["--cache_order", "1"], "need --cache_blocks"),
    (["--cache_blocks", "2", "--dpm_solver", "ode"], "exclusive"),
    (["--cache_blocks", "2", "--clip_x0"], "exclusive"),
    (["--cache_blocks", "2", "--dynamic_threshold", "0.995"], "exclusive"),
    (["--cache_blocks", "2", "--resample_jump", "2", "--resample_count", "2"], "exclusive"),
    (["--cache_blocks", "2", "--restart", "100", "500", "1"], "exclusive"),
    (["--cache_blocks", "2", "--pag_scale", "1"], "exclusive"),
    (["--cache_blocks", "2", "--autoguidance_scale", "1"], "exclusive"),
])
def test_validate_cache_rejects_before_any_gpu_work(extra, match):
    from duodiff_amd import sampler
    from duodiff_amd.config import load_config
    args = sampler.get_args(cli_argv(CELEBA, *extra))
    with pytest.raises(ValueError, match=match):
        sampler.validate_cache(args, load_config(CELEBA))


def test_validate_cache_a_pair_and_the_defaults():
    from duodiff_amd import sampler
    from duodiff_amd.config import load_config
    cfg, cfg3 = load_config(CELEBA), load_config(CELEBA_3)
    a = sampler.get_args(cli_argv(CELEBA))
    assert a.cache_blocks is None and a.cache_interval is None and a.cache_order is None
    assert sampler.validate_cache(a, cfg) is None
    assert sampler.validate_cache(sampler.get_args(cli_argv(CELEBA, "--cache_blocks", "2")), cfg) == (2, 3, 0)
    assert sampler.validate_cache(sampler.get_args(cli_argv(CELEBA, "--cache_blocks", "6", "--cache_interval", "5", "--cache_order", "1")),
                                       cfg) == (6, 5, 1)
    pair = sampler.get_args(cli_argv(CELEBA_3, "--checkpoint_path_late", "/nonexistent.pth", "--config_path_late", str(CELEBA), "--cache_blocks", "2"))
    with pytest.raises(ValueError, match="depth"):          # the first model has depth 3: depth // 2 = 1
        sampler.validate_cache(pair, cfg3, cfg)
    with pytest.raises(SystemExit):
        sampler.get_args(cli_argv(CELEBA, "--cache_blocks", "2", "--cache_order", "2"))


def test_cli_main_rejects_cache_blocks_before_it_builds_a_model(tmp_path):
    from duodiff_amd import sampler
    argv = cli_argv(CELEBA, "--cache_blocks", "7")
    argv[argv.index("--output_folder") + 1] = str(tmp_path / "out")
    with pytest.raises(ValueError, match="depth"):
        sampler.main(argv)


def test_get_samples_rejects_before_any_engine_call():
    """get_samples' own rejections, the early-exit models among them: the stand-in models have no engine_model to call"""
    from duodiff_amd import sampler

    class Plain:
        depth, device = 5, "cpu"

    class EarlyExit(Plain):
        classifier_type = "attention_probe"

    common = dict(batch_size=2, postprocessing=sampler.predict_noise_postprocessing, seed=3, num_channels=3, sample_height=8, sample_width=8, num_steps=7)
    cases = [(dict(model=EarlyExit(), cache=(1, 3, 0)), "early-exit"),
             (dict(model=Plain(), late_model=EarlyExit(), t_switch=4, cache=(1, 3, 0)), "early-exit"),
             (dict(model=Plain(), cache=(1, 3, 0), pag=(1.0, [0], [0])), "combine"),
             (dict(model=Plain(), late_model=Plain(), t_switch=4, cache=(1, 3, 0), autoguidance_scale=1.0), "combine"),
             (dict(model=Plain(), cache=(3, 3, 0)), "depth"),
             (dict(model=Plain(), cache=(1, 3, 2)), "cache_order")]
    for noise in ("device", "torch_cpu"):
        for kw, match in cases:
            with pytest.raises(ValueError, match=match):
                sampler.get_samples(noise=noise, **common, **kw)
    with pytest.raises(AttributeError, match="engine_model"):          # (what passes the checks goes on to the engine)
        sampler.get_samples(Plain(), cache=(2, 3, 0), **common)


def test_eesampler_does_not_take_the_options():
    from duodiff_amd import eesampler
    assert "cache_blocks" not in (REPO / "duodiff_amd" / "eesampler.py").read_text() and hasattr(eesampler, "main")


# ---- the binding ---------------------------------------------------------------------------------------------------------------
def test_lib_binds_the_cached_entry_points():
    assert L.ABI_VERSION == 6
    assert C.sizeof(L.dd_block_cache) == 24
    assert C.sizeof(L.dd_affine_sample_args) == 104
    op, w = (C.c_int32 * 2)(0, 2), (C.c_float * 2)(0.0, 0.5)
    bc = L.dd_block_cache(2, 1, op, w)
    assert bc.blocks == 2 and bc.order == 1 and bc.op[1] == 2 and bc.w[1] == 0.5
    assert L.SIGNATURES["dd_forward_cached"][1] == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.POINTER(L.dd_guidance),
                                                    C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_int, C.c_void_p]
    assert L.SIGNATURES["dd_sample_affine_cached"][1] == [C.c_void_p, C.POINTER(L.dd_affine_sample_args), C.POINTER(L.dd_guidance),
                                                          C.POINTER(L.dd_known_region), C.POINTER(L.dd_block_cache), C.c_void_p]
    lib = L.load()
    assert lib.dd_abi_version() == 6
    for name in ("dd_forward_cached", "dd_sample_affine_cached", "dd_dev_cache_extrapolate"):
        assert hasattr(lib, name)
    from duodiff_amd import engine
    assert hasattr(engine.Model, "forward_cached") and hasattr(engine, "sample_affine_cached_loop")


# ---- the gate of the kernel test -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("sigma", [1.0, 100.0])
@pytest.mark.parametrize("w", [0.5, 1.0, -0.25, 2.0])
def test_the_kernel_gate_rejects_wrong_results(w, sigma, prec):
    """The elementwise gate of the kernel test on the CPU: the float64 result rounded to the activation type passes; prev and last swapped,
    w negated, and last alone where w = 1 do not."""
    last, prev = extrapolate_operands(64, 256, sigma, prec, 7)
    ref, tol = extrapolate_ref(last, prev, w, prec)
    rnd = bf16 if prec == "bf16" else (lambda a: a)
    assert gate(rnd(ref.astype(np.float32)), ref, tol, "the rounded reference") <= 1.0
    # the kernel's own order of operations in fp32, each step rounded: inside the bound too
    d = (last - prev).astype(np.float32)
    y = (last + (np.float32(w) * d).astype(np.float32)).astype(np.float32)
    assert gate(rnd(y), ref, tol, "fp32 in the kernel's order") <= 1.0
    wrong = {"swapped": extrapolate_ref(prev, last, w, prec)[0], "negated": extrapolate_ref(last, prev, -w, prec)[0]}
    if w == 1.0:
        wrong["last alone"] = last.astype(np.float64)
    for what, bad in wrong.items():
        with pytest.raises(AssertionError):
            gate(rnd(bad.astype(np.float32)), ref, tol, what)
