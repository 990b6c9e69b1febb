"""threshold_scan's host side (no GPU): the numpy mirror of scan_tanh_abs against float64 tanh, the replay of the sampler's exit rule against the
oracle's, the statistics and the suggestion on constructed arrays, the option checks."""
import argparse

import numpy as np
import pytest

from duodiff_amd import threshold_scan as ts
from oracle.early_exit_oracle import early_exit_select
from scan_support import E_TANH, TANH_BREAKPOINTS

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- the mirror
def test_tanh_mirror_against_float64_on_a_strided_sweep():
    """every 7919th fp32 value (a prime: no pattern of the mantissa is favoured) from 0 to the clamp, the neighbourhood of both breakpoints,
    denormals, values past the clamp and inf.  E_TANH itself comes from the full sweep (tools/scan_tanh_sweep.py)."""
    assert E_TANH <= 1e-6
    top = int(F32(ts.TANH_CLAMP).view(np.uint32))
    bits = [np.arange(0, top + 1, 7919, dtype=np.uint32)]
    for bp in TANH_BREAKPOINTS:
        c = int(F32(bp).view(np.uint32))
        bits.append(np.arange(max(c - 4096, 0), c + 4096, dtype=np.uint32))
    bits.append(np.arange(0, 1 << 16, dtype=np.uint32))                                   # 0 and the smallest denormals
    bits.append(np.arange((1 << 23) - 2048, (1 << 23) + 2048, dtype=np.uint32))           # the largest denormals, the smallest normals
    x = np.concatenate(bits).view(F32)
    x = np.concatenate([x, np.array([1.1165210, 10.5, 11.0, 100.0, 3e38, np.inf], F32)])
    r = ts.tanh_abs_f32(x)
    assert r.dtype == F32 and (r >= 0).all() and (r <= 1).all()
    err = np.abs(r.astype(np.float64) - np.tanh(x.astype(np.float64)))
    print(f"{x.size} values: max error {err.max():.4e} at {float(x[err.argmax()])!r} (E_TANH {E_TANH:.3e})")
    assert err.max() <= E_TANH
    assert ts.tanh_abs_f32(F32(0)) == 0 and ts.tanh_abs_f32(F32(-0.0)) == 0
    assert np.array_equal(ts.tanh_abs_f32(-x).view(np.uint32), r.view(np.uint32))         # even in d
    assert (np.diff(ts.tanh_abs_f32(np.linspace(0, 12, 4001).astype(F32)).astype(np.float64)) >= -2 * E_TANH).all()


def test_tanh_mirror_uses_float32_arithmetic_only():
    """a float64 intermediate would show: the result differs from the float64 evaluation of the same rational in a fraction of the values"""
    x = np.linspace(0.01, 9.0, 20001).astype(F32)
    h = 0.5 * x.astype(np.float64)
    s = h * h
    t = h * (((s + 378) * s + 17325) * s + 135135) / (((28 * s + 3150) * s + 62370) * s + 135135)
    exact = np.minimum(2 * t / (1 + t * t), 1.0)
    r = ts.tanh_abs_f32(x)
    assert (r != exact.astype(F32)).mean() > 0.05
    assert np.abs(r - exact).max() < 5e-7


# ---------------------------------------------------------------------------------------------------------------- the exit rule
@pytest.mark.parametrize("seed", range(4))
def test_simulate_exits_is_the_oracles_selection(seed):
    r = np.random.default_rng(seed)
    n, depth, N = 3, 5, 64
    pred = r.uniform(-0.1, 0.6, (n, depth, N)).astype(F32)
    pred[0, :, :8] = r.uniform(0.3, 0.6, (depth, 8))               # columns that never exit early at the thresholds below
    pred[1, 2, 5] = -0.05                                          # a negative prediction
    thresholds = [0.0, 0.25, float(pred[2, 1, 7]), float(pred[0, 3, 9]), float(np.nextafter(pred[2, 1, 7], F32(-1))), 1.0, 0.1 + 1e-9, -0.01]
    for thr in thresholds:
        idx = ts.simulate_exits(pred, thr)
        assert idx.shape == (n, N)
        for k in range(n):
            eps = np.zeros((N, 1), F32)
            outs = [np.zeros((N, 1), F32)] * depth
            want = early_exit_select(eps, list(pred[k]), outs, thr)[1]
            assert np.array_equal(idx[k], want), (thr, k)
    # an entry equal to the threshold to the bit exits there; one ulp below the entry it does not
    thr = float(pred[2, 1, 7])
    col = pred[2, :, 7]
    first = int(np.argmax(np.append(col, F32(0)) <= F32(thr)))
    assert ts.simulate_exits(pred, thr)[2, 7] == first <= 1
    # the float32 comparison: a threshold that rounds to the entry as float32 exits although the double is smaller
    assert ts.simulate_exits(pred, thr - 1e-12)[2, 7] == first
    # all False (a negative threshold): 0, the reference's argmax quirk
    assert (ts.simulate_exits(np.full((1, depth, 4), 0.5, F32), -1.0) == 0).all()
    assert (ts.simulate_exits(np.full((1, depth, 4), 0.5, F32), 0.0) == depth).all()


# ---------------------------------------------------------------------------------------------------------------- statistics and the suggestion
def _tables(n=4, depth=3, N=16, seed=0):
    r = np.random.default_rng(seed)
    mse = r.uniform(0.5, 1.5, (n, depth + 1, N))
    return mse


def test_identical_exits_give_gap_zero_and_the_largest_candidate():
    mse = _tables()
    mse[:] = mse[:, -1:, :]                                        # every exit is as good as the backbone
    thresholds = [0.0, 0.1, 0.2, 0.4]
    r = np.random.default_rng(1)
    gaps, sems = [], []
    for _ in thresholds:
        idx = r.integers(0, mse.shape[1], (mse.shape[0], mse.shape[2]))
        gap, sem, blocks = ts.threshold_statistics(mse, idx)
        assert (gap == 0).all() and (sem == 0).all() and 0 <= blocks <= 1
        gaps.append(gap); sems.append(sem)
    assert ts.suggest_threshold(thresholds, gaps, sems, tolerance=0.0, sems=2.0) == 0.4
    assert ts.suggest_threshold(thresholds[::-1], gaps, sems, tolerance=0.0, sems=2.0) == 0.4      # the order of the list does not matter


def test_threshold_statistics_values():
    n, depth, N = 2, 3, 4
    mse = np.arange(n * (depth + 1) * N, dtype=np.float64).reshape(n, depth + 1, N) + 1.0
    idx = np.array([[0, 1, 2, 3], [3, 3, 3, 3]])
    gap, sem, blocks = ts.threshold_statistics(mse, idx)
    realised0 = np.array([mse[0, 0, 0], mse[0, 1, 1], mse[0, 2, 2], mse[0, 3, 3]])
    d0 = realised0 - mse[0, 3]
    assert gap[0] == pytest.approx(d0.mean() / mse[0, 3].mean()) and gap[1] == 0
    assert sem[0] == pytest.approx(d0.std(ddof=1) / 2 / mse[0, 3].mean()) and sem[1] == 0
    assert blocks == pytest.approx((0 + 1 + 2 + 3 + 12) / 8 / 3)
    assert ts.threshold_statistics(mse, np.full((n, N), depth))[2] == 1.0
    with pytest.raises(ValueError):
        ts.threshold_statistics(mse, np.full((n, N), depth + 1))
    with pytest.raises(ValueError):
        ts.threshold_statistics(mse, idx[:1])


def test_one_bad_timestep_blocks_a_candidate_and_every_candidate_above_it():
    thresholds = [0.05, 0.1, 0.2, 0.3]
    gaps = np.zeros((4, 5))
    sems = np.full((4, 5), 0.001)
    gaps[2, 3] = 0.5                                               # candidate 0.2 fails at one timestep only
    assert ts.suggest_threshold(thresholds, gaps, sems, tolerance=0.02) == 0.1       # 0.3 is acceptable on its own and still not suggested
    gaps[2, 3] = 0.0185                                            # the standard error decides: 0.0185 + 2 * 0.001 > 0.02
    assert ts.suggest_threshold(thresholds, gaps, sems, tolerance=0.02) == 0.1
    assert ts.suggest_threshold(thresholds, gaps, sems, tolerance=0.02, sems=1.0) == 0.3
    gaps[0, 0] = 1.0
    assert ts.suggest_threshold(thresholds, gaps, sems, tolerance=0.02) is None      # the smallest fails: the backbone alone
    assert ts.suggest_threshold(thresholds, np.ones((4, 5)), sems, tolerance=0.02) is None
    with pytest.raises(ValueError):
        ts.suggest_threshold(thresholds, gaps[:3], sems[:3], 0.02)


def test_calibration_values():
    r = np.random.default_rng(3)
    target = r.uniform(0.1, 0.9, (5, 4, 7))
    pred = target[:, :3] * 0.5 + 0.1                                # an exact linear relation: r = 1
    cal = ts.calibration(pred, target)
    assert np.allclose(cal["pearson_r"], 1.0) and len(cal["rmse"]) == 3
    assert np.allclose(cal["mean_predicted"], pred.mean(axis=(0, 2))) and np.allclose(cal["mean_target"], target[:, :3].mean(axis=(0, 2)))
    assert np.allclose(cal["rmse"], np.sqrt(((pred - target[:, :3]) ** 2).mean(axis=(0, 2))))
    assert np.isnan(ts.calibration(np.ones((2, 1, 3)), target[:2, :1, :3])["pearson_r"][0])


def test_candidate_thresholds():
    pred = np.linspace(-0.2, 0.8, 1001).astype(F32).reshape(1, 1, -1)
    q = ts.candidate_thresholds(pred, num_thresholds=32)
    assert q[0] == 0.0 and q == sorted(set(q)) and len(q) <= 32 and all(float(F32(v)) == v for v in q) and q[-1] == float(F32(0.8))
    assert ts.candidate_thresholds(pred, thresholds=[0.3, 0.1, 0.1]) == [float(F32(0.1)), float(F32(0.3))]
    for bad in ([-0.1], [float("nan")], [float("inf")], []):
        with pytest.raises(ValueError):
            ts.candidate_thresholds(pred, thresholds=bad)
    with pytest.raises(ValueError):
        ts.candidate_thresholds(pred)                                              # neither
    with pytest.raises(ValueError):
        ts.candidate_thresholds(pred, thresholds=[0.1], num_thresholds=4)          # both
    with pytest.raises(ValueError):
        ts.candidate_thresholds(pred, num_thresholds=0)


# ---------------------------------------------------------------------------------------------------------------- options
CONFIG = {"model_params": dict(img_size=16, patch_size=2, in_chans=3, embed_dim=64, depth=3, num_heads=2, num_classes=-1,
                               normalize_timesteps=True, classifier_type="mlp_probe_per_layer")}


def _args(tmp_path, **kw):
    np.save(tmp_path / "x.npy", np.zeros((2, 3, 16, 16), F32))
    base = dict(seed=0, config_path="c.yaml", checkpoint_path="c.pth", parametrization="predict_noise", images=str(tmp_path / "x.npy"),
                class_label=None, labels=None, timesteps=[999, 0], stride=None, thresholds=None, num_thresholds=None, repeats=1, tolerance=0.02,
                sems=2.0, batch_size=2, output_folder=str(tmp_path), precision="bf16", no_graph=False)
    base.update(kw)
    return argparse.Namespace(**base)


def test_option_validation(tmp_path):
    a = _args(tmp_path)
    assert ts.validate(a, CONFIG) == [999, 0] and a.num_thresholds == 32           # the default
    assert ts.validate(_args(tmp_path, parametrization="predict_original", thresholds=[0.0, 0.1]), CONFIG) == [999, 0]
    bad = [dict(parametrization="predict_previous"), dict(thresholds=[-0.1]), dict(thresholds=[float("nan")]), dict(thresholds=[float("inf")]),
           dict(thresholds=[0.1], num_thresholds=8), dict(num_thresholds=0), dict(timesteps=[5, 5]), dict(timesteps=[1000]),
           dict(timesteps=None), dict(stride=10), dict(repeats=0), dict(tolerance=-1.0), dict(sems=float("nan")), dict(seed=-1),
           dict(class_label=1), dict(images=str(tmp_path / "missing.txt")), dict(batch_size=0)]
    for kw in bad:
        with pytest.raises(ValueError):
            ts.validate(_args(tmp_path, **kw), CONFIG)
    plain = {"model_params": {k: v for k, v in CONFIG["model_params"].items() if k != "classifier_type"}}
    with pytest.raises(ValueError, match="classifier_type"):
        ts.validate(_args(tmp_path), plain)
    cond = {"model_params": dict(CONFIG["model_params"], num_classes=10)}
    with pytest.raises(ValueError, match="class-conditional"):
        ts.validate(_args(tmp_path), cond)
    assert ts.validate(_args(tmp_path, class_label=3), cond) == [999, 0]
    p = ts.get_args(["--config_path", "c", "--checkpoint_path", "p", "--parametrization", "predict_noise", "--images", "i", "--stride", "100",
                     "--output_folder", "o"])
    assert p.thresholds is None and p.num_thresholds is None and p.stride == 100
