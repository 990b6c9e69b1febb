"""Per-image seeds without a GPU: the command-line flags of sampler / dist / eesampler, the seed arithmetic, the per-image label draw,
the rejections that come before any GPU work, the binding and the headers.  The GPU half is tests/test_image_seeds.py."""
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from duodiff_amd import _lib as L
from duodiff_amd import dist, eesampler, sampler
from loop_support import cli_argv

CFG = REPO / "configs" / "uvit_celeba_3.yaml"
NEW_SYMBOLS = ("dd_set_image_seeds", "dd_noise_images", "dd_dev_final_seeded")


def test_flags_and_defaults():
    a = sampler.get_args(cli_argv(CFG))
    assert a.image_seeds is False and a.first_image == 0
    assert sampler.image_seed_list(a, 2) is None
    a = sampler.get_args(cli_argv(CFG, "--image_seeds", "--first_image", "7", "--seed", "100"))
    assert a.image_seeds is True and a.first_image == 7
    e = eesampler.get_args(["--threshold", "0.1", "--checkpoint_path", "x", "--batch_size", "3", "--output_folder", "o", "--config_path", "c"])
    assert e.image_seeds is False and e.first_image == 0
    e = eesampler.get_args(["--threshold", "0.1", "--checkpoint_path", "x", "--batch_size", "3", "--output_folder", "o", "--config_path", "c",
                            "--image_seeds", "--first_image", "4", "--noise", "device"])
    assert e.image_seeds and e.first_image == 4 and sampler.image_seed_list(e, 3) == [4, 5, 6]


def test_seed_arithmetic():
    a = sampler.get_args(cli_argv(CFG, "--image_seeds", "--first_image", "7", "--seed", "100"))
    assert sampler.image_seed_list(a, 3) == [107, 108, 109]                 # image i of the run: --seed + N + i
    assert sampler.image_seed_list(a, 1, first_image=9) == [109]
    # a run of W ranks x B is the run of W B images: rank r starts at N + r B under the SAME base seed
    B, W = 4, 3
    whole = sampler.image_seed_list(a, W * B)
    shards = [sampler.image_seed_list(a, B, dist.rank_first_image(a.first_image, r, B)) for r in range(W)]
    assert sum(shards, []) == whole
    assert dist.rank_first_image(7, 0, 4) == 7 and dist.rank_first_image(7, 2, 4) == 15
    assert dist.rank_seed(11, 2) == 13                                       # without the flag: as before


def test_sample_sharded_keeps_the_base_seed_under_image_seeds(monkeypatch):
    seen = []
    fn = lambda seed: seen.append(seed) or torch.zeros(1, 2, 2, 3)
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("WORLD_SIZE", "1")
    dist.sample_sharded(fn, 11, rank_seeds=False)
    dist.sample_sharded(fn, 11)
    assert seen == [11, 11]
    monkeypatch.setattr(dist, "env_rank", lambda: (3, 1, 0))                 # (a world of 1 gathers nothing: only the seed is looked at)
    dist.sample_sharded(fn, 11, rank_seeds=False)
    dist.sample_sharded(fn, 11)
    assert seen[2:] == [11, 14]


def test_rejections_before_any_gpu_work():
    with pytest.raises(ValueError, match="--noise device"):
        sampler.validate_image_seeds(sampler.get_args(cli_argv(CFG, "--image_seeds", "--noise", "torch_cpu")))
    with pytest.raises(ValueError, match="--noise device"):                   # eesampler's default noise is torch_cpu
        sampler.validate_image_seeds(eesampler.get_args(["--threshold", "0.1", "--checkpoint_path", "x", "--batch_size", "3", "--output_folder", "o",
                                                         "--config_path", "c", "--image_seeds"]))
    with pytest.raises(ValueError, match="--image_seeds"):
        sampler.validate_image_seeds(sampler.get_args(cli_argv(CFG, "--first_image", "2")))
    with pytest.raises(ValueError, match="negative"):
        sampler.validate_image_seeds(sampler.get_args(cli_argv(CFG, "--image_seeds", "--first_image", "-1")))
    sampler.validate_image_seeds(sampler.get_args(cli_argv(CFG, "--image_seeds")))              # --noise device is the sampler's default
    sampler.validate_image_seeds(sampler.get_args(cli_argv(CFG)))
    kw = dict(model=None, batch_size=2, postprocessing=sampler.predict_noise_postprocessing, seed=0, num_channels=3, sample_height=8, sample_width=8)
    with pytest.raises(ValueError, match="noise='device'"):
        sampler.get_samples(**kw, noise="torch_cpu", image_seeds=[1, 2])
    with pytest.raises(ValueError, match="3 seeds"):
        sampler.get_samples(**kw, noise="device", image_seeds=[1, 2, 3])


def test_label_draw_is_a_function_of_the_image_seed_alone():
    a = sampler.get_args(cli_argv(CFG, "--image_seeds", "--class_id", "3", "--seed", "40"))
    seeds = sampler.image_seed_list(a, 5)
    torch.manual_seed(1)
    y = sampler.labels_from_args(a, 5, 1001, seeds)
    torch.manual_seed(2)                                                      # the global stream does not enter
    assert torch.equal(y, sampler.labels_from_args(a, 5, 1001, seeds))
    assert y.dtype == torch.int64 and int(y.min()) >= 1 and int(y.max()) <= 1000 and len(set(y.tolist())) > 1
    for i, s in enumerate(seeds):                                             # any slice, any order: label i from seed i
        assert torch.equal(sampler.draw_labels_per_image([s], 1001), y[i:i + 1])
        assert int(y[i]) == int(torch.randint(1, 1001, (1,), generator=torch.Generator().manual_seed(s)))
    assert torch.equal(sampler.draw_labels_per_image(seeds[::-1], 1001), y.flip(0))
    with pytest.raises(IndexError):
        sampler.draw_labels_per_image(seeds, 10)                              # the reference's range check
    # --class_label is unaffected; without image seeds the draw is the reference's
    b = sampler.get_args(cli_argv(CFG, "--image_seeds", "--class_label", "3"))
    assert sampler.labels_from_args(b, 4, 10, [1, 2, 3, 4]).tolist() == [3, 3, 3, 3]
    torch.manual_seed(5)
    want = torch.randint(1, 1001, (4,))
    torch.manual_seed(5)
    assert torch.equal(sampler.labels_from_args(a, 4, 1001), want)


def test_binding_and_abi():
    assert L.ABI_VERSION == 6
    for name in NEW_SYMBOLS:
        assert name in L.SIGNATURES
    assert len(L.SIGNATURES["dd_set_image_seeds"][1]) == 3 and len(L.SIGNATURES["dd_noise_images"][1]) == 9
    assert len(L.SIGNATURES["dd_dev_final_seeded"][1]) == len(L.SIGNATURES["dd_dev_final"][1]) + 2
    lib = L.load()
    assert lib.dd_abi_version() == 6
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
    assert lib.dd_set_image_seeds(None, None, 0) == L.DD_ERR_INVALID and lib.dd_noise_images(None, 0, None, 0, None, 1, 1, 1, None) == L.DD_ERR_INVALID


def test_headers_declare_the_symbols_and_keep_the_structs():
    pub, dev = (REPO / "include" / "duodiff.h").read_text(), (REPO / "include" / "duodiff_dev.h").read_text()
    assert re.search(r"#define DD_ABI_VERSION 6\b", pub)
    assert re.search(r"int dd_set_image_seeds\(dd_ctx\* ctx, const uint64_t\* seeds_dev, int n\);", pub)
    assert re.search(r"int dd_noise_images\(dd_ctx\* ctx, uint64_t seed, const uint64_t\* seeds_dev, int counter, float\* out_dev, int B, int C, "
                     r"int S, void\* stream\);", pub)
    assert re.search(r"int dd_dev_final_seeded\(dd_ctx\* ctx, dd_dev_final_args\* args, const uint64_t\* seeds_host, int n, void\* stream\);", dev)
    assert "seeds" not in re.search(r"typedef struct dd_dev_final_args \{.*?\} dd_dev_final_args;", dev, re.S).group(0)


def test_draw_site_is_the_only_pixel_id_arithmetic():
    """step.hip's drawing kernels take (key, id) from step_update.h draw_site: no philox_normal4 call names st->seed or a batch-wide id itself"""
    step = (REPO / "duodiff_amd" / "csrc" / "step.hip").read_text()
    calls = re.findall(r"philox_normal4\(([^;]*);", step)
    assert len(calls) >= 6
    for c in calls:
        assert c.startswith("ds.key, ds.id, "), c
    assert step.count("draw_site(") == 5        # z and z2 of the output head, the thresholded step, the early-exit step, x_T
    hdr = (REPO / "duodiff_amd" / "csrc" / "step_update.h").read_text()
    assert "PHILOX_START" in hdr and len({w for w in re.findall(r"PHILOX_\w+ = (0x[0-9a-f]+)u", hdr)}) == 3
