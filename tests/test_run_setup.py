"""The run setup the sampler's two command lines share (sampler.setup_run): python -m duodiff_amd.sampler and python -m duodiff_amd.dist
build the same models on the same rows and hand get_samples the same keyword arguments, for every option dist takes; dist refuses the
options it does not take before it builds anything.

CPU: sampler.build_model and sampler.get_samples are recorders, the configs are YAML files of the test.  GPU: the two command lines,
in process and on one rank, write the same samples.npy under --pag_scale and under --clip_x0, and not the pictures of the run without
the option.
"""
import numpy as np
import pytest
import torch
import yaml

from conftest import REPO, TINY
from duodiff_amd import dist, sampler
from duodiff_amd.config import ModelParams
from loop_support import cli_argv

CONFIGS = REPO / "configs"
FILES = {"pixel": dict(TINY), "cond": dict(TINY, num_classes=1001), "shallow": dict(TINY, depth=1), "full": dict(TINY, depth=3)}


@pytest.fixture
def files(tmp_path):
    for name, cfg in FILES.items():
        (tmp_path / f"{name}.yaml").write_text(yaml.safe_dump({"model_params": cfg}))
    return tmp_path


class _FakeModel:
    device = "cpu"


def _argv(files, config, *extra, late=None):
    argv = ["--seed", "5", "--checkpoint_path", f"{config}.pth", "--batch_size", "2", "--parametrization", "predict_noise", "--output_folder",
            str(files / "out"), "--config_path", str(files / f"{config}.yaml"), "--no_png", *extra]
    if late is not None:
        argv += ["--checkpoint_path_late", f"{late}.pth", "--config_path_late", str(files / f"{late}.yaml"), "--t_switch", "300"]
    return argv


def _record(monkeypatch, main, argv):
    """main(argv) with recorders for build_model and get_samples -> (the build_model calls, the get_samples keyword arguments)"""
    builds, calls = [], []

    def build_model(config, checkpoint_path, precision, max_batch):
        builds.append((config, checkpoint_path, precision, max_batch))
        m = _FakeModel()
        m.name = checkpoint_path
        return m, ModelParams.from_dict(config)

    def get_samples(*args, **kw):
        assert not args
        calls.append(kw)
        images = torch.zeros(kw["batch_size"], 8, 8, 3)
        return (images if kw.get("return_device_tensor") else images.numpy()), []
    monkeypatch.setattr(sampler, "build_model", build_model)
    monkeypatch.setattr(sampler, "get_samples", get_samples)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    main(argv)
    assert len(calls) == 1
    return builds, calls[0]


def _same(a, b):
    if isinstance(a, _FakeModel):
        return isinstance(b, _FakeModel) and a.name == b.name
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and torch.equal(a, b)
    return type(a) is type(b) and a == b


RUNS = {
    "plain": ("pixel", [], None, 2),
    "cfg": ("cond", ["--cfg_scale", "0.4", "--class_label", "207"], None, 4),
    "cfg-class_id-pair": ("cond", ["--cfg_scale", "1.5", "--class_id", "3", "--cfg_null_label", "999", "--use_ddim", "--ddim_steps", "7"], "cond", 4),
    "autoguidance-pair": ("shallow", ["--autoguidance_scale", "1.0"], "full", 2),
    "autoguidance-explicit": ("full", ["--autoguidance_scale", "0.5", "--guide_config_path", "shallow.yaml", "--guide_checkpoint_path", "guide.pth"],
                              None, 2),
    "pag": ("pixel", ["--pag_scale", "3"], None, 4),
    "pag-pair": ("shallow", ["--pag_scale", "2", "--pag_layers", "0", "mid", "--pag_layers_first", "0", "--no_graph"], "full", 4),
    "clip": ("pixel", ["--clip_x0"], None, 2),
    "dynamic": ("pixel", ["--dynamic_threshold", "0.9", "--threshold_max", "2", "--precision", "fp32"], None, 2),
    "solver": ("shallow", ["--dpm_solver", "sde", "--dpm_solver_steps", "9", "--dpm_solver_order", "1"], "full", 2),
    "image_seeds": ("cond", ["--image_seeds", "--first_image", "4", "--class_id", "1", "--dpm_solver", "ode"], None, 2),
    "torch_cpu": ("pixel", ["--noise", "torch_cpu", "--parametrization", "predict_original"], None, 2),
}


@pytest.mark.parametrize("name", sorted(RUNS))
def test_both_command_lines_set_the_same_run_up(monkeypatch, files, name):
    config, extra, late, rows = RUNS[name]
    extra = [str(files / v) if v.endswith(".yaml") else v for v in extra]
    argv = _argv(files, config, *extra, late=late)
    builds_s, kw_s = _record(monkeypatch, sampler.main, argv)
    builds_d, kw_d = _record(monkeypatch, dist.main, argv)
    assert builds_s == builds_d and len(builds_s) == 1 + (late is not None) + ("--guide_config_path" in extra)
    assert [b[3] for b in builds_s] == [rows] * len(builds_s)
    assert [b[1] for b in builds_s] == [f"{config}.pth"] + ([f"{late}.pth"] if late else []) + (["guide.pth"] if "guide.pth" in extra else [])
    assert sorted(kw_s) == sorted(set(kw_d) - {"return_device_tensor"})
    for key in kw_s:
        if key != "timesteps_save":
            assert _same(kw_s[key], kw_d[key]), key
    assert kw_s["timesteps_save"] == [] and kw_d["timesteps_save"] == [] and kw_d["return_device_tensor"] is True
    # the options arrive: what the flag asks for is in the call, not its default
    a = sampler.get_args(argv)
    assert kw_d["cfg_scale"] == a.cfg_scale and kw_d["autoguidance_scale"] == a.autoguidance_scale
    assert (kw_d["pag"] is None) == (a.pag_scale is None) and (kw_d["threshold"] is None) == (a.clip_x0 is None and a.dynamic_threshold is None)
    assert (kw_d["guide_model"] is None) == (a.guide_config_path is None) and (kw_d["image_seeds"] is None) == (not a.image_seeds)
    assert (kw_d["y"] is None) == (a.class_id is None and a.class_label is None) and kw_d["seed"] == 5


def test_the_shared_arguments(monkeypatch, files):
    """what the options become: guidance pairs and masks, the threshold record, the solver's names, the seeds of the run's images"""
    _, kw = _record(monkeypatch, dist.main, _argv(files, "shallow", *RUNS["pag-pair"][1], late="full"))
    assert kw["pag"] == (2.0, [0], [0, 1]) and kw["use_graph"] is False and kw["t_switch"] == 300
    assert kw["model"].name == "shallow.pth" and kw["late_model"].name == "full.pth" and kw["guide_model"] is None
    assert kw["postprocessing"] is sampler.predict_noise_postprocessing
    assert (kw["num_channels"], kw["sample_height"], kw["sample_width"], kw["batch_size"]) == (3, 8, 8, 2)
    _, kw = _record(monkeypatch, dist.main, _argv(files, "pixel", *RUNS["dynamic"][1]))
    assert kw["threshold"] == sampler.X0Threshold("dynamic", quantile=0.9, s_max=2.0)
    _, kw = _record(monkeypatch, dist.main, _argv(files, "full", "--autoguidance_scale", "0.5", "--guide_config_path",
                                                   str(files / "shallow.yaml"), "--guide_checkpoint_path", "guide.pth"))
    assert kw["guide_model"].name == "guide.pth" and kw["autoguidance_scale"] == 0.5
    _, kw = _record(monkeypatch, dist.main, _argv(files, "cond", *RUNS["image_seeds"][1]))
    assert kw["image_seeds"] == [9, 10] and kw["solver"] == "dpmsolver++" and kw["y"].shape == (2,)
    _, kw = _record(monkeypatch, sampler.main, _argv(files, "pixel", "--timesteps_save", "10", "500"))
    assert kw["timesteps_save"] == [10, 500] and "return_device_tensor" not in kw


REGION_FLAGS = [["--init_image", "i.npy"], ["--strength", "0.5"], ["--known_image", "k.npy"], ["--known_mask", "m.npy"], ["--encode_images"]]


@pytest.mark.parametrize("extra,match", [(f, "belong to the single-GPU sampler") for f in REGION_FLAGS]
                         + [(["--timesteps_save", "10"], "--timesteps_save belongs to the single-GPU sampler")])
def test_dist_refuses_what_it_does_not_do(monkeypatch, files, extra, match):
    def no_model(*a, **k):
        raise AssertionError("a model was built")
    monkeypatch.setattr(sampler, "build_model", no_model)
    monkeypatch.setattr(dist, "init", no_model)
    with pytest.raises(ValueError, match=match):
        dist.main(_argv(files, "pixel", *extra))


_LATE = ["--checkpoint_path_late", "/nonexistent.pth", "--config_path_late"]
# the argv of the command line's rejection tests (test_guidance, test_autoguidance, test_pag, test_x0_threshold, test_multistep)
REJECTED = [
    ("uvit_celeba.yaml", ["--cfg_scale", "0.4", "--class_id", "3"]),
    ("uvit_imagenet64.yaml", ["--cfg_scale", "0.4", "--class_label", "3"]),
    ("uvit_imagenet256.yaml", ["--cfg_scale", "0.4"]),
    ("uvit_imagenet256.yaml", ["--class_label", "1001"]),
    ("uvit_imagenet256.yaml", ["--class_label", "-1"]),
    ("uvit_celeba.yaml", ["--class_label", "3"]),
    ("uvit_imagenet256.yaml", ["--cfg_scale", "0.4", "--class_label", "3", "--cfg_null_label", "1001"]),
    ("uvit_imagenet256.yaml", ["--cfg_scale", "nan", "--class_label", "3"]),
    ("uvit_imagenet256_3.yaml", ["--cfg_scale", "0.4", "--class_label", "3", *_LATE, str(CONFIGS / "uvit_imagenet64.yaml")]),
    ("uvit_celeba_3.yaml", ["--autoguidance_scale", "nan", *_LATE, str(CONFIGS / "uvit_celeba.yaml")]),
    ("uvit_celeba_3.yaml", ["--autoguidance_scale", "inf", *_LATE, str(CONFIGS / "uvit_celeba.yaml")]),
    ("uvit_imagenet256_3.yaml", ["--autoguidance_scale", "1", "--cfg_scale", "0.4", "--class_label", "3", *_LATE, str(CONFIGS / "uvit_imagenet256.yaml")]),
    ("uvit_celeba_3.yaml", ["--autoguidance_scale", "1", *_LATE, str(CONFIGS / "uvit_cifar10.yaml")]),
    ("uvit_celeba.yaml", ["--autoguidance_scale", "1", "--guide_config_path", str(CONFIGS / "uvit_imagenet256_3.yaml"), "--guide_checkpoint_path",
                          "/nonexistent.pth"]),
    ("uvit_celeba.yaml", ["--autoguidance_scale", "1"]),
    ("uvit_celeba.yaml", ["--autoguidance_scale", "1", "--guide_config_path", str(CONFIGS / "uvit_celeba_3.yaml")]),
    ("uvit_celeba.yaml", ["--guide_config_path", str(CONFIGS / "uvit_celeba_3.yaml"), "--guide_checkpoint_path", "/nonexistent.pth"]),
    ("uvit_celeba.yaml", ["--pag_scale", "1", "--pag_layers", "13"]),
    ("uvit_celeba.yaml", ["--pag_scale", "1", "--pag_layers", "middle"]),
    ("uvit_celeba.yaml", ["--pag_scale", "nan"]),
    ("uvit_celeba.yaml", ["--pag_layers", "3"]),
    ("uvit_celeba.yaml", ["--pag_scale", "1", "--pag_layers_first", "1"]),
    ("uvit_imagenet256.yaml", ["--pag_scale", "1", "--cfg_scale", "0.4", "--class_label", "3"]),
    ("uvit_celeba.yaml", ["--pag_scale", "1", "--clip_x0"]),
    ("uvit_celeba.yaml", ["--pag_scale", "1", "--dynamic_threshold", "0.995"]),
    ("uvit_celeba_3.yaml", ["--pag_scale", "1", "--autoguidance_scale", "1.0", *_LATE, str(CONFIGS / "uvit_celeba.yaml")]),
    ("uvit_celeba.yaml", ["--clip_x0", "--dynamic_threshold", "0.9"]),
    ("uvit_celeba.yaml", ["--clip_x0", "0"]),
    ("uvit_celeba.yaml", ["--clip_x0", "inf"]),
    ("uvit_celeba.yaml", ["--dynamic_threshold", "0"]),
    ("uvit_celeba.yaml", ["--dynamic_threshold", "1.5"]),
    ("uvit_celeba.yaml", ["--dynamic_threshold", "0.9", "--threshold_max", "0.5"]),
    ("uvit_celeba.yaml", ["--threshold_max", "2"]),
    ("uvit_celeba.yaml", ["--clip_x0", "--threshold_max", "2"]),
    ("uvit_imagenet256.yaml", ["--clip_x0"]),
    ("uvit_celeba.yaml", ["--dynamic_threshold", "0.9", "--parametrization", "predict_previous"]),
    ("uvit_celeba.yaml", ["--clip_x0", "--noise", "torch_cpu"]),
    ("uvit_celeba.yaml", ["--dpm_solver", "ode", "--use_ddim"]),
    ("uvit_celeba.yaml", ["--dpm_solver", "sde", "--parametrization", "predict_previous"]),
    ("uvit_celeba.yaml", ["--dpm_solver", "ode", "--dpm_solver_steps", "0"]),
    ("uvit_celeba.yaml", ["--image_seeds", "--noise", "torch_cpu"]),
    ("uvit_celeba.yaml", ["--first_image", "2"]),
]


@pytest.mark.parametrize("config,extra", REJECTED, ids=[f"{i}{e[0]}" for i, (_, e) in enumerate(REJECTED)])
def test_dist_rejects_what_the_sampler_rejects(monkeypatch, tmp_path, config, extra):
    def no_model(*a, **k):
        raise AssertionError("a model was built")
    monkeypatch.setattr(sampler, "build_model", no_model)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    argv = cli_argv(CONFIGS / config, *extra)
    argv[argv.index("--output_folder") + 1] = str(tmp_path / "out")
    with pytest.raises(ValueError) as want:
        sampler.main(argv)
    with pytest.raises(ValueError) as got:
        dist.main(argv)
    assert str(got.value) == str(want.value)


def test_backbone_rows():
    assert sampler.backbone_rows(6) == 6 and sampler.backbone_rows(6, cfg_scale=0.0) == 12 and sampler.backbone_rows(6, pag=(0.0, [1], [])) == 12
    assert sampler.backbone_rows(6, None, None) == 6


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_files(tmp_path_factory):
    from duodiff_amd.weights import synthetic_state_dict
    d = tmp_path_factory.mktemp("run_setup")
    cfg = dict(TINY, img_size=16, depth=3)
    (d / "m.yaml").write_text(yaml.safe_dump({"model_params": cfg}))
    torch.save(dict(synthetic_state_dict(ModelParams.from_dict(cfg), 17)), d / "m.pth")
    return d


def _cli_samples(main, d, out, *extra):
    main(["--seed", "3", "--checkpoint_path", str(d / "m.pth"), "--config_path", str(d / "m.yaml"), "--parametrization", "predict_noise",
          "--precision", "fp32", "--noise", "device", "--use_ddim", "--ddim_steps", "5", "--batch_size", "2", "--no_png",
          "--output_folder", str(d / out), *extra])
    return (d / out / "samples.npy").read_bytes()


@pytest.fixture(scope="module")
def plain_samples(gpu_files):
    return _cli_samples(sampler.main, gpu_files, "plain")


@pytest.mark.gpu
@pytest.mark.parametrize("option", [["--pag_scale", "2.0"], ["--clip_x0"]], ids=["pag", "clip_x0"])
def test_dist_honours_the_option_like_the_sampler(monkeypatch, gpu_files, plain_samples, option):
    """single-rank dist writes the sampler's samples.npy byte for byte, and not the file of the run without the option (which is what it
    wrote while it dropped the option)"""
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("RANK", raising=False)
    tag = option[0].strip("-")
    one = _cli_samples(sampler.main, gpu_files, f"sampler_{tag}", *option)
    sharded = _cli_samples(dist.main, gpu_files, f"dist_{tag}", *option)
    assert sharded == one
    assert one != plain_samples and np.isfinite(np.load(gpu_files / f"dist_{tag}" / "samples.npy")).all()
