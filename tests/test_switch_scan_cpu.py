"""The denoising-error scan, host side (no GPU): step_plan.scan_rows against float64 restatements of the reference's trainer, the rule
that turns paired errors into a t_switch, every rejection of the command line before a model is built, the layout of scan.json, and the
binding of the new entry points against both headers."""
import ctypes as C
import json
import re
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import REPO
from duodiff_amd import _lib as L
from duodiff_amd import scan_common, step_plan, switch_scan
from duodiff_amd.config import load_config
from duodiff_amd.engine import schedule_tables

CONFIGS = REPO / "configs"
GRID = [999, 998, 700, 500, 1, 0]


# ---- scan_rows -----------------------------------------------------------------------------------------------------------------
def _tables64():
    return {k: v.astype(np.float64) for k, v in schedule_tables().items()}


@pytest.mark.parametrize("par", ["predict_noise", "predict_original", "predict_previous"])
def test_scan_rows_against_float64_restatements(par):
    """x_t = sqrt(abar) x0 + sqrt(1 - abar) z (the scheduler's add_noise) and the trainer's target coefficients (trainer.py:319-352), in
    float64 from the bit-exact tables and rounded once"""
    tb = _tables64()
    r = step_plan.scan_rows(GRID, par)
    assert set(r) == {"t", "ka", "kb", "tz", "t0", "tx"} and all(v.dtype == np.float32 and v.shape == (len(GRID),) for v in r.values())
    assert r["t"].tolist() == [float(t) for t in GRID]
    for k, t in enumerate(GRID):
        ab, ab_p, beta, alpha = tb["alphas_bar"][t], tb["alphas_bar_previous"][t], tb["betas"][t], tb["alphas"][t]
        assert r["ka"][k] == np.float32(np.sqrt(ab)) and r["kb"][k] == np.float32(np.sqrt(1.0 - ab))
        want = {"predict_noise": (1.0, 0.0, 0.0), "predict_original": (0.0, 1.0, 0.0),
                "predict_previous": (0.0, np.sqrt(ab_p) * beta / (1.0 - ab), np.sqrt(alpha) * (1.0 - ab_p) / (1.0 - ab))}[par]
        assert (r["tz"][k], r["t0"][k], r["tx"][k]) == tuple(np.float32(v) for v in want)
    if par == "predict_previous":      # t = 0: the previous image is the clean one (1 - abar[0] carries abar's fp32 rounding: 2^-24 / 1e-4 = 6e-4)
        assert abs(r["t0"][-1] - 1.0) < 1e-3 and r["tx"][-1] == 0.0
        assert 0 < r["t0"][0] < 1e-3 and 0.98 < r["tx"][0] < 1.0


def test_scan_rows_ka_kb_equal_known_rows():
    """exactly what known_rows gives a step that lands on t"""
    ka, kb = step_plan.known_rows(SimpleNamespace(lands=tuple(GRID)))
    r = step_plan.scan_rows(GRID, "predict_noise")
    assert np.array_equal(r["ka"], ka) and np.array_equal(r["kb"], kb)


@pytest.mark.parametrize("ts,par", [([], "predict_noise"), ([1000], "predict_noise"), ([-1], "predict_noise"), ([5], "predict_eps"), ([[1, 2]], "predict_noise")])
def test_scan_rows_rejects(ts, par):
    with pytest.raises(ValueError):
        step_plan.scan_rows(ts, par)


# ---- suggest_t_switch ------------------------------------------------------------------------------------------------------------
TS = [999, 900, 800, 700, 600, 500, 0]


def _errors(gaps, n=64, noise=0.0, seed=0):
    """late errors of 1 + small per-image spread; first = late (1 + gap_k) + noise * N(0, 1) per image"""
    r = np.random.default_rng(seed)
    late = 1.0 + 0.01 * r.standard_normal((len(gaps), n))
    first = late * (1.0 + np.asarray(gaps)[:, None]) + noise * r.standard_normal((len(gaps), n))
    return first, late


def test_suggest_the_300_case():
    """acceptable on 999 .. 700, not at 600: t_min = 700 and the sampler's t_switch = 300 runs the first model on 999 .. 700"""
    first, late = _errors([0.0, 0.001, 0.002, 0.004, 0.08, 0.3, 2.0])
    assert switch_scan.suggest_t_switch(TS, first, late, tolerance=0.02) == 300
    # the order of the rows does not matter, and an acceptable timestep below a rejected one does not count
    perm = [3, 0, 6, 2, 5, 1, 4]
    assert switch_scan.suggest_t_switch([TS[i] for i in perm], first[perm], late[perm], tolerance=0.02) == 300
    first2, late2 = _errors([0.0, 0.001, 0.002, 0.004, 0.08, 0.0, 0.0])
    assert switch_scan.suggest_t_switch(TS, first2, late2, tolerance=0.02) == 300
    # every timestep acceptable, 0 on the grid: the first model everywhere
    first3, late3 = _errors([0.0] * 7)
    assert switch_scan.suggest_t_switch(TS, first3, late3, tolerance=0.02) == 1000
    gap, sem = scan_common.gap_statistics(first, late)
    d = first - late
    assert np.allclose(gap, d.mean(1) / late.mean(1), rtol=1e-14) and np.allclose(sem, d.std(1, ddof=1) / 8.0 / late.mean(1), rtol=1e-14)


def test_suggest_a_noisy_gap_only_the_sems_term_rejects():
    """mean gap 0.01 <= 0.02 at t = 800, but the paired differences are noisy: sem ~ 0.5 / 8 -> rejected with sems = 2, accepted with sems = 0"""
    gaps = [0.0, 0.0, 0.01, 0.0, 0.5, 0.5, 0.5]
    first, late = _errors(gaps, n=64, seed=3)
    noise = np.random.default_rng(4).standard_normal(64)
    first[2] = late[2] + 0.01 * late[2].mean() + 0.5 * (noise - noise.mean())
    gap, sem = scan_common.gap_statistics(first, late)
    assert gap[2] <= 0.02 < gap[2] + 2 * sem[2]
    assert switch_scan.suggest_t_switch(TS, first, late, tolerance=0.02, sems=2.0) == 100
    assert switch_scan.suggest_t_switch(TS, first, late, tolerance=0.02, sems=0.0) == 300


def test_suggest_none_and_a_grid_without_999():
    first, late = _errors([0.05, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    assert switch_scan.suggest_t_switch(TS, first, late, tolerance=0.02) is None          # not 0: to the sampler that is "first model everywhere"
    with pytest.raises(ValueError, match="999"):
        switch_scan.suggest_t_switch(TS[1:], first[1:], late[1:], tolerance=0.02)
    with pytest.raises(ValueError):
        switch_scan.suggest_t_switch(TS, first, late[:, :5], tolerance=0.02)
    with pytest.raises(ValueError, match="distinct"):
        switch_scan.suggest_t_switch([999] * 7, first, late, tolerance=0.02)
    one_f, one_l = _errors([0.0] * 7, n=1)
    assert switch_scan.suggest_t_switch(TS, one_f, one_l, tolerance=0.02) == 1000           # one image: no spread to add


def test_scan_timesteps():
    assert scan_common.scan_timesteps(stride=250) == [999, 749, 499, 249]
    assert scan_common.scan_timesteps(stride=333) == [999, 666, 333, 0]
    assert scan_common.scan_timesteps(stride=5000) == [999]
    assert scan_common.scan_timesteps(timesteps=[5, 999, 0]) == [5, 999, 0]
    for kw in (dict(), dict(timesteps=[1], stride=2), dict(stride=0), dict(timesteps=[1000]), dict(timesteps=[-1]), dict(timesteps=[3, 3])):
        with pytest.raises(ValueError):
            scan_common.scan_timesteps(**kw)


# ---- the command line ------------------------------------------------------------------------------------------------------------
def _argv(config, tmp_path, *extra, images=None, grid=("--stride", "100")):
    if images is None:
        images = tmp_path / "x.npy"
    return ["--config_path", str(CONFIGS / config), "--checkpoint_path", "/nonexistent.pth", "--parametrization", "predict_noise",
            "--images", str(images), "--output_folder", str(tmp_path / "out"), *grid, *extra]


PAIR = ["--config_path_late", str(CONFIGS / "uvit_celeba.yaml"), "--checkpoint_path_late", "/nonexistent.pth"]


@pytest.mark.parametrize("config,extra,grid,match", [
    ("uvit_celeba.yaml", [], (), "one of them"),
    ("uvit_celeba.yaml", ["--timesteps", "5"], ("--stride", "10"), "one of them"),
    ("uvit_celeba.yaml", [], ("--stride", "0"), "stride"),
    ("uvit_celeba.yaml", [], ("--timesteps", "1000"), "999"),
    ("uvit_celeba.yaml", [], ("--timesteps", "7", "7"), "twice"),
    ("uvit_celeba.yaml", ["--seed", "-1"], ("--stride", "100"), "seed"),
    ("uvit_celeba.yaml", ["--repeats", "0"], ("--stride", "100"), "repeats"),
    ("uvit_celeba.yaml", ["--batch_size", "0"], ("--stride", "100"), "batch_size"),
    ("uvit_celeba.yaml", ["--tolerance", "nan"], ("--stride", "100"), "tolerance"),
    ("uvit_celeba.yaml", ["--tolerance", "-0.1"], ("--stride", "100"), "tolerance"),
    ("uvit_celeba.yaml", ["--sems", "inf"], ("--stride", "100"), "sems"),
    ("uvit_celeba.yaml", ["--config_path_late", str(CONFIGS / "uvit_celeba.yaml")], ("--stride", "100"), "go together"),
    ("uvit_celeba.yaml", ["--class_label", "3"], ("--stride", "100"), "class-conditional"),
    ("uvit_celeba.yaml", ["--labels", "y.npy"], ("--stride", "100"), "class-conditional"),
    ("uvit_imagenet64.yaml", [], ("--stride", "100"), "class-conditional"),
    ("uvit_imagenet64.yaml", ["--class_label", "3", "--labels", "y.npy"], ("--stride", "100"), "exclusive"),
    ("uvit_imagenet64.yaml", ["--class_label", "100000"], ("--stride", "100"), "outside"),
    ("uvit_celeba.yaml", ["--encode_images"], ("--stride", "100"), "latent"),
    ("uvit_celeba.yaml", ["--encode_mean"], ("--stride", "100"), "encode_images"),
    ("uvit_celeba_3.yaml", PAIR, ("--timesteps", "900", "500"), "999"),
    ("uvit_cifar10_3.yaml", PAIR, ("--stride", "100"), "disagree"),
])
def test_validate_rejects_before_any_gpu_work(tmp_path, config, extra, grid, match):
    """validate against the YAMLs alone: no image is read, no model is built, no GPU is touched"""
    args = switch_scan.get_args(_argv(config, tmp_path, *extra, grid=grid))
    late = load_config(args.config_path_late) if args.config_path_late else None
    with pytest.raises(ValueError, match=match):
        switch_scan.validate(args, load_config(args.config_path), late)


def test_validate_rejects_image_sources(tmp_path):
    (tmp_path / "pngs").mkdir()
    for config, images, extra, match in (("uvit_celeba.yaml", tmp_path / "x.txt", [], "folder"),
                                         ("uvit_imagenet256.yaml", tmp_path / "pngs", ["--class_label", "1"], "latent"),):
        args = switch_scan.get_args(_argv(config, tmp_path, *extra, images=images))
        with pytest.raises(ValueError, match=match):
            switch_scan.validate(args, load_config(args.config_path))
    # accepted: the grid comes back
    args = switch_scan.get_args(_argv("uvit_celeba_3.yaml", tmp_path, *PAIR, grid=("--stride", "300")))
    assert switch_scan.validate(args, load_config(args.config_path), load_config(args.config_path_late)) == [999, 699, 399, 99]
    args = switch_scan.get_args(_argv("uvit_imagenet256.yaml", tmp_path, "--class_label", "1", "--encode_images", images=tmp_path / "pngs"))
    assert switch_scan.validate(args, load_config(args.config_path))[0] == 999
    assert args.tolerance == 0.02 and args.sems == 2.0 and args.repeats == 1 and not args.no_graph


def test_images_and_labels_must_fit_the_model(tmp_path):
    from duodiff_amd.config import ModelParams
    mp = ModelParams.from_dict(load_config(CONFIGS / "uvit_celeba.yaml"))
    for shape, ok in (((2, 3, 64, 64), True), ((2, 3, 32, 32), False), ((2, 1, 64, 64), False), ((3, 64, 64), False), ((0, 3, 64, 64), False)):
        np.save(tmp_path / "x.npy", np.zeros(shape, np.float32))
        args = switch_scan.get_args(_argv("uvit_celeba.yaml", tmp_path))
        if ok:
            assert scan_common.load_images(args.images, mp.in_chans, mp.img_size).shape == shape
        else:
            with pytest.raises(ValueError, match="resized"):
                scan_common.load_images(args.images, mp.in_chans, mp.img_size)
    np.save(tmp_path / "x.npy", np.full((1, 3, 64, 64), np.nan, np.float32))
    with pytest.raises(ValueError, match="finite"):
        scan_common.load_images(switch_scan.get_args(_argv("uvit_celeba.yaml", tmp_path)).images, mp.in_chans, mp.img_size)
    # PNGs: through evaluation.read_samples, then 2 v - 1
    from PIL import Image
    (tmp_path / "pngs").mkdir()
    px = np.random.default_rng(1).integers(0, 256, (64, 64, 3), dtype=np.uint8)
    Image.fromarray(px).save(tmp_path / "pngs" / "a.png")
    got = scan_common.load_images(switch_scan.get_args(_argv("uvit_celeba.yaml", tmp_path, images=tmp_path / "pngs")).images, mp.in_chans, mp.img_size)
    assert got.shape == (1, 3, 64, 64) and np.array_equal(got[0], 2.0 * (px.transpose(2, 0, 1).astype(np.float32) / 255.0) - 1.0)
    # labels
    args = switch_scan.get_args(_argv("uvit_imagenet64.yaml", tmp_path, "--class_label", "7"))
    assert scan_common.load_labels(args, 3, 1000).tolist() == [7, 7, 7]
    np.save(tmp_path / "y.npy", np.array([1, 2, 999]))
    args = switch_scan.get_args(_argv("uvit_imagenet64.yaml", tmp_path, "--labels", str(tmp_path / "y.npy")))
    assert scan_common.load_labels(args, 3, 1000).dtype == np.int64
    for n, classes in ((4, 1000), (3, 999)):
        with pytest.raises(ValueError):
            scan_common.load_labels(args, n, classes)
    assert scan_common.load_labels(switch_scan.get_args(_argv("uvit_celeba.yaml", tmp_path)), 3, -1) is None


def test_main_rejects_before_it_builds_a_model(tmp_path):
    with pytest.raises(ValueError, match="one of them"):
        switch_scan.main(_argv("uvit_celeba.yaml", tmp_path, grid=()))
    with pytest.raises(SystemExit):                                             # the early-exit form is not part of this version
        switch_scan.get_args(_argv("uvit_celeba.yaml", tmp_path, "--early_exit"))


def test_json_layout(tmp_path):
    grid = [999, 700, 400]
    args = switch_scan.get_args(_argv("uvit_celeba_3.yaml", tmp_path, *PAIR, "--repeats", "2", "--tolerance", "0.05", grid=("--timesteps", "999", "700", "400")))
    r = np.random.default_rng(0)
    late = 1.0 + 0.01 * r.standard_normal((2, 3, 8))
    first = late * (1.0 + np.array([0.0, 0.01, 0.5])[None, :, None])
    err = np.stack([first, late]).astype(np.float32)                            # [models, repeats, n, N]
    s = switch_scan.summarize(args, grid, err, ["first", "late"])
    s = json.loads(json.dumps(s))
    assert set(s) == {"parametrization", "timesteps", "images", "repeats", "seed", "precision", "models", "gap", "sem", "acceptable", "tolerance",
                      "sems", "t_switch", "advice"}
    assert s["timesteps"] == grid and s["images"] == 8 and s["repeats"] == 2 and s["tolerance"] == 0.05 and s["sems"] == 2.0
    assert set(s["models"]) == {"first", "late"} and all(len(m["mean_error"]) == 3 for m in s["models"].values())
    per = err.astype(np.float64).mean(1)
    assert np.allclose(s["models"]["late"]["mean_error"], per[1].mean(1), rtol=1e-12)
    assert np.allclose(s["gap"], (per[0] - per[1]).mean(1) / per[1].mean(1), rtol=1e-12)
    assert s["acceptable"] == [True, True, False] and s["t_switch"] == 300 and s["advice"] == "--t_switch 300"
    assert s["t_switch"] == switch_scan.suggest_t_switch(grid, per[0], per[1], 0.05, 2.0)
    # a single model: the means alone; a pair that misses at 999: null and the advice says so
    single = json.loads(json.dumps(switch_scan.summarize(args, grid, err[:1], ["first"])))
    assert "gap" not in single and "t_switch" not in single and set(single["models"]) == {"first"}
    miss = json.loads(json.dumps(switch_scan.summarize(args, grid, np.stack([late * 2, late]).astype(np.float32), ["first", "late"])))
    assert miss["t_switch"] is None and "late model alone" in miss["advice"]


# ---- the binding -----------------------------------------------------------------------------------------------------------------
def test_signatures_declared_in_both_headers():
    """dd_scan_error in include/duodiff.h, the two dev entries in include/duodiff_dev.h, each bound in _lib.SIGNATURES with the struct laid
    out field for field; the ABI stays 6"""
    assert L.ABI_VERSION == 6
    pub, dev = (REPO / "include" / "duodiff.h").read_text(), (REPO / "include" / "duodiff_dev.h").read_text()
    assert "#define DD_ABI_VERSION 6" in pub
    assert re.search(r"int dd_scan_error\(dd_ctx\* ctx, const dd_scan_args\* args, void\* stream\);", pub)
    assert "dd_dev_scan" not in pub
    for name in ("dd_dev_scan_diffuse", "dd_dev_scan_error"):
        assert re.search(rf"int {name}\(dd_ctx\* ctx, dd_dev_scan_args\* args,", dev) and name in L.SIGNATURES
    assert L.SIGNATURES["dd_scan_error"] == (C.c_int, [C.c_void_p, C.POINTER(L.dd_scan_args), C.c_void_p])
    assert L.SIGNATURES["dd_dev_scan_diffuse"][1] == [C.c_void_p, C.POINTER(L.dd_dev_scan_args), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    assert L.SIGNATURES["dd_dev_scan_error"][1] == [C.c_void_p, C.POINTER(L.dd_dev_scan_args), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]

    def fields(text, struct):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                names += [v.strip().lstrip("*").strip() for v in re.sub(r"^(const )?(unsigned long long|[A-Za-z_0-9]+)\*?\s", "", decl).split(",")]
        return names

    assert fields(pub, "dd_scan_args") == [f[0] for f in L.dd_scan_args._fields_]
    assert fields(dev, "dd_dev_scan_args") == [f[0] for f in L.dd_dev_scan_args._fields_]
    assert C.sizeof(L.dd_scan_args) == 112 and L.dd_scan_args.err_dev.offset == 104 and L.dd_scan_args.seed.offset == 80
    assert C.sizeof(L.dd_dev_scan_args) == 88 and L.dd_dev_scan_args.seed.offset == 56
    lib = L.load()
    assert lib.dd_abi_version() == 6
    for name in ("dd_scan_error", "dd_dev_scan_diffuse", "dd_dev_scan_error"):
        assert hasattr(lib, name)
    from duodiff_amd import engine
    assert callable(engine.scan_error_loop)
    # engine._run_loop puts the image tensor into the field its caller names: x0_dev for the scans, whose structs have no x_dev
    from types import SimpleNamespace as NS
    assert "x_dev" not in dict(L.dd_scan_args._fields_) and "x_dev" not in dict(L.dd_scan_exits_args._fields_)
    image, ctx, seen = NS(data_ptr=lambda: 4096, shape=(3, 1, 2, 2), device=None), NS(check=lambda rc: None), []
    for a in (L.dd_scan_args(), L.dd_scan_exits_args()):
        engine._run_loop(ctx, a, image, None, 7, "philox", False, NS(cuda_stream=64), lambda st: seen.append(st.value), image="x0_dev")
        assert a.x0_dev == 4096 and (a.B, a.seed, a.y_dev, a.noise_mode, a.use_graph) == (3, 7, None, L.DD_NOISE_PHILOX, 0)
    a = L.dd_sample_args()
    engine._run_loop(ctx, a, image, None, 7, "none", False, NS(cuda_stream=64), lambda st: seen.append(st.value))
    assert a.x_dev == 4096 and seen == [64, 64, 64]
