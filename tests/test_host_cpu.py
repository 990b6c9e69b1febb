"""CPU: host-side logic, the C-ABI library's exports and its host-only arithmetic.
No GPU compute here; the product has no CPU path, which is itself asserted."""
import ctypes
import re

import numpy as np
import pytest
import torch

from conftest import FULL_NAMES, REPO, TINY, have_gpu
from duodiff_amd import _lib
from duodiff_amd.config import ModelParams, load_config
from duodiff_amd.weights import num_params, param_shapes, synthetic_state_dict


def test_library_exports_every_declared_symbol():
    # the drop-in boundary (duodiff.h) and the development / validation entry points (duodiff_dev.h, dd_dev_* only)
    header = (REPO / "include" / "duodiff.h").read_text()
    dev = (REPO / "include" / "duodiff_dev.h").read_text()
    declared = set(re.findall(r"\b(dd_[a-z_0-9]+)\s*\(", header))
    declared -= {"dd_ctx", "dd_model", "dd_vae"}
    assert not any(n.startswith("dd_dev_") for n in declared), "development entry points belong in duodiff_dev.h"
    dev_declared = set(re.findall(r"\b(dd_dev_[a-z_0-9]+)\s*\(", dev))
    lib = _lib.load()
    assert declared | dev_declared == set(_lib.SIGNATURES), (declared | dev_declared) ^ set(_lib.SIGNATURES)
    for name in declared | dev_declared:
        assert hasattr(lib, name), name
    assert lib.dd_abi_version() == _lib.ABI_VERSION


def test_engine_schedule_tables_bit_exact_with_reference(golden):
    from duodiff_amd.engine import schedule_tables
    fx = golden("schedule.npz")
    t = schedule_tables()
    for k in ("betas", "alphas", "alphas_bar", "alphas_bar_previous", "betas_tilde"):
        assert np.array_equal(t[k], fx["sampler_" + k]), k
    assert np.array_equal(t["betas_tilde_scheduler"], fx["sched_betas_tilde"])
    assert t["sigma"][0] == 0.0 and abs(t["c1"][999] - 1.01015) < 1e-5 and abs(t["c2"][999] - 0.02) < 1e-6


def test_schedule_mirrors():
    from duodiff_amd import sampler
    from duodiff_amd.ddpm_core import NoiseScheduler
    s = NoiseScheduler()
    assert torch.equal(s.betas, sampler.schedule.betas) and s.sigma_squared() is s.betas
    assert NoiseScheduler(variance_mode="beta_tilde").sigma_squared().shape == (1000,)
    with pytest.raises(ValueError):                      # raised where the reference raises it (ddpm_core.py:72-79)
        NoiseScheduler(variance_mode="nope").sigma_squared()
    # any schedule: bit-equal to the oracle's restatement of ddpm_core.py:64-70 (pinned by schedule.npz at 1000 steps)
    import oracle
    for args in ((1e-4, 0.02, 50), (1e-4, 0.02, 1000), (3e-4, 0.05, 333), (1e-4, 0.02, 7)):
        s = NoiseScheduler(*args, variance_mode="beta_tilde")
        want = oracle.scheduler_schedule(*args)
        for k in ("betas", "alphas", "alphas_bar", "alpha_bar_prev", "betas_tilde"):
            assert np.array_equal(getattr(s, k).numpy(), want[k]), (args, k)
        t = args[2] // 2
        c1, c2, sg = s.step_coefficients(t)
        o1, o2, o3 = oracle.schedule_oracle.step_coefficients(want, t, "beta_tilde")
        assert (np.float32(c1), np.float32(c2), np.float32(sg)) == (o1, o2, o3)


@pytest.mark.skipif(have_gpu(), reason="asserts the no-GPU failure mode")
def test_no_cpu_fallback():
    from duodiff_amd.engine import Context
    from duodiff_amd.uvit import UViT
    with pytest.raises(_lib.EngineUnavailable):
        Context()
    h = ctypes.c_void_p()
    assert _lib.load().dd_ctx_create(0, ctypes.byref(h)) != 0 and not h.value
    mp = ModelParams.from_dict(dict(TINY))
    m = UViT(**mp.as_dict())
    m.load_state_dict(synthetic_state_dict(mp, 1))
    with pytest.raises(Exception):
        m(torch.zeros(1, 3, 8, 8), torch.zeros(1))


def test_configs_load_and_match_survey_inventory():
    want = {"uvit_cifar10": 44255328, "uvit_cifar10_3": 10122848, "uvit_celeba": 44292228,
            "uvit_celeba_3": 10159748, "uvit_imagenet64": 130940292, "uvit_imagenet64_3": 23479428,
            "uvit_imagenet256": 286763172, "uvit_imagenet256_3": 41202852}
    gflop = {"uvit_cifar10": 24.402, "uvit_celeba": 24.421, "uvit_celeba_3": 5.552, "uvit_imagenet64": 70.472,
             "uvit_imagenet256": 152.912, "uvit_imagenet256_3": 21.396}
    for name in FULL_NAMES:
        mp = ModelParams.from_dict(load_config(REPO / "configs" / f"{name}.yaml"))  # extra keys tolerated (Q3)
        assert num_params(mp) == want[name], name
        assert mp.seq_len in (257, 258) and mp.head_dim == 64 and mp.num_patches == 256
        if name in gflop:
            assert abs(mp.flops_per_image() / 1e9 - gflop[name]) < 2e-3, name
    with pytest.raises(FileNotFoundError):
        load_config(REPO / "configs" / "does_not_exist.yaml")


def test_synthetic_weights_are_seeded_and_complete():
    mp = ModelParams.from_dict(dict(TINY, num_classes=10))
    a, b, c = synthetic_state_dict(mp, 3), synthetic_state_dict(mp, 3), synthetic_state_dict(mp, 4)
    assert list(a) == list(param_shapes(mp))
    assert all(torch.equal(a[k], b[k]) for k in a) and not torch.equal(a["pos_embed"], c["pos_embed"])
    assert "label_emb.weight" in a and a["out_blocks.0.skip_linear.weight"].shape == (64, 128)
    assert float(a["mid_block.mlp.fc1.bias"].abs().max()) > 0  # biases randomised (reference init zeroes them)


def test_load_state_dict_surface():
    from duodiff_amd.uvit import UViT
    mp = ModelParams.from_dict(dict(TINY))
    sd = synthetic_state_dict(mp, 1)
    m = UViT(**mp.as_dict(), classifier_type="mlp_per_layer")  # unknown key ignored (quirk Q3)
    m.load_state_dict({"model_state_dict": sd, "step": 7})      # trainer checkpoint format
    assert list(m.state_dict()) == list(sd)
    bad = dict(sd)
    bad.pop("norm.weight")
    with pytest.raises(RuntimeError):
        UViT(**mp.as_dict()).load_state_dict(bad)
    bad = dict(sd)
    bad["pos_embed"] = torch.zeros(1, 3, 64)
    with pytest.raises(RuntimeError):
        UViT(**mp.as_dict()).load_state_dict(bad)
    # the two constructor options no shipped YAML uses are part of the schema (models/uvit.py:150, 264-272)
    mp2 = ModelParams.from_dict(dict(mp.as_dict(), mlp_time_embed=True, qkv_bias=True))
    keys = set(param_shapes(mp2)) - set(param_shapes(mp))
    assert {"time_embed.0.weight", "time_embed.0.bias", "time_embed.2.weight", "time_embed.2.bias", "mid_block.attn.qkv.bias"} <= keys
    with pytest.raises(RuntimeError):                      # a checkpoint without them does not load into such a model
        UViT(**mp2.as_dict()).load_state_dict(sd)


def test_cli_arguments_match_reference_surface():
    from duodiff_amd import sampler
    a = sampler.get_args(["--checkpoint_path", "a.pth", "--batch_size", "4", "--parametrization", "predict_noise",
                          "--output_folder", "o", "--config_path", "c.yaml"])
    assert a.seed == 0 and a.t_switch == np.inf and a.checkpoint_path_late is None and a.config_path_late is None
    assert a.class_id is None and a.use_ddim is False and a.ddim_steps == 50 and a.ddim_eta == 0.0
    assert a.timesteps_save == [] and a.precision == "bf16"
    with pytest.raises(SystemExit):
        sampler.get_args(["--batch_size", "4"])
    assert a.noise == "device" and a.no_graph is False


def test_model_param_validation_through_c_abi():
    """dd_model_create / set_param argument checking is host-only, but needs a ctx -> GPU; here we
    only check that bad configs are rejected by the Python mirror before reaching the device."""
    with pytest.raises(ValueError):
        ModelParams.from_dict(dict(TINY, depth=4))
    with pytest.raises(ValueError):
        ModelParams.from_dict(dict(TINY, img_size=9))
    with pytest.raises(KeyError):
        ModelParams.from_dict({"img_size": 8})


def test_gemm_row_partition_covers_every_row_once_and_fills_the_cus():
    """The 256x256 GEMM's row partition (host arithmetic in libduodiff.so): q*256 main rows + e tail rows per
    tile cover [0, M) exactly once, and for the BASELINE shapes the tile counts are exact multiples of 256 CUs."""
    lib = _lib.load()
    q, e = ctypes.c_int(), ctypes.c_int()

    def plan(M, N, K, cus=256):
        rc = lib.dd_plan_rows(M, N, K, cus, ctypes.byref(q), ctypes.byref(e))
        return (q.value, e.value) if rc == 0 else None

    for B, L, D in ((128, 257, 512), (256, 258, 768), (32, 258, 1024), (100, 257, 512), (2, 257, 512)):
        M = B * L
        for N, K in ((D, D), (3 * D, D), (4 * D, D), (D, 4 * D), (D, 2 * D)):
            if N % 256:
                assert plan(M, N, K) is None
                continue
            qq, ee = plan(M, N, K)
            assert 0 <= ee <= 8 and qq >= 1 and 256 * qq <= M
            covered = np.zeros(M, np.int32)
            for t in range(qq):
                covered[256 * t: 256 * (t + 1)] += 1
                lo = 256 * qq + t * ee
                covered[lo: min(M, lo + ee)] += 1
            assert (covered == 1).all(), (B, L, N, K, qq, ee)
    # CelebA B=128: 256 / 768 / 1024 tiles -> 1 / 3 / 4 exact rounds on 256 CUs
    for N, tiles in ((512, 256), (1536, 768), (2048, 1024)):
        qq, ee = plan(128 * 257, N, 512)
        assert (qq, ee) == (128, 1) and qq * (N // 256) == tiles
    # ImageNet-64 B=256, L=258: 2 tail rows per tile instead of 258 M-tiles
    assert plan(256 * 258, 768, 768) == (256, 2)
    assert plan(100, 512, 512) is None and plan(1024, 48, 512) is None      # tiny M / narrow N fall back


def test_bench_roofline_leg_follows_the_committed_kernel_table():
    """bench.py times the kernel that rocprofv3's committed table of the workload ranks first: the block tail on the
    headline workload, the row-resident Linear on ImageNet-64, the split-K GEMM on the ImageNet-256 latents -- and every family it can
    select has a FLOP / byte model and a DD_PROF_* kind the library accepts."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", REPO / "bench.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    from duodiff_amd.engine import Model
    want = {"celeba": "block_tail", "imagenet64": "rowlin", "imagenet256": "splitk"}
    for w, (_, _, cfg_f, B, _) in b.WORKLOADS.items():
        mp = ModelParams.from_dict(load_config(REPO / "configs" / f"{cfg_f}.yaml"))
        shares = b.kernel_shares(w)
        assert shares and shares[0][0] == want[w], (w, shares)
        assert abs(sum(s for _, _, s in shares)) <= 1.0 + 1e-9
        for kind, frag, share in shares:
            fl, by, pmc, name, n = b.family_model(kind, mp, B)
            assert fl > 0 and by > 0 and n > 0 and frag in pmc + name
            assert kind in Model.PROFILE_KINDS and 0 < b.cu_share_half_batch(kind, mp, B) <= 1.0
    lib = _lib.load()
    assert lib.dd_profile_select(None, 0) == _lib.DD_ERR_INVALID      # (a null context is refused: the symbol exists and checks its arguments)
    # ... and so is it by the single-kernel development entry points (csrc/dev_harness.hip), called through their bound signatures with every
    # pointer null and every integer 0: they check the context before anything touches the GPU
    for name in ("dd_dev_mlp", "dd_dev_block_tail", "dd_dev_qkv_attention", "dd_dev_qkv_attention_rows", "dd_dev_head_dec", "dd_dev_gemm", "dd_dev_rowlin", "dd_dev_attention",
                 "dd_dev_layernorm", "dd_dev_embed", "dd_dev_time_mlp", "dd_dev_final", "dd_dev_vae_gather", "dd_dev_groupnorm", "dd_dev_softmax_rows", "dd_dev_vae_input",
                 "dd_dev_vae_output", "dd_dev_vae_moments", "dd_dev_cast", "dd_dev_vae_trace", "dd_dev_ee_probe", "dd_dev_ee_probe_reduce", "dd_dev_ee_attn_probe"):
        args = [0 if t in (ctypes.c_int, ctypes.c_longlong, ctypes.c_size_t) else 0.0 if t is ctypes.c_float else None for t in _lib.SIGNATURES[name][1]]
        assert getattr(lib, name)(*args) == _lib.DD_ERR_INVALID, name


def test_bench_steps_and_output_dump(tmp_path):
    """--steps K runs exactly K timed steps (runs of at most 1000, the 30 / 70 mix in each) and --dump-outputs stays under 64 MB with a
    fixed sample of whole images when the output is larger."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", REPO / "bench.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert b.sampling_runs(20, 300) == [(20, 6)] and b.sampling_runs(1000, 300) == [(1000, 300)]
    assert b.sampling_runs(2500, 300) == [(1000, 300), (1000, 300), (500, 150)] and b.sampling_runs(1, 300) == [(1, 1)]
    for K in (1, 7, 999, 1000, 1001, 3999, 4000):
        assert sum(k for k, _ in b.sampling_runs(K, 300)) == K
    assert b.parse(["--steps", "3", "--dump-outputs", str(tmp_path)]).dump_outputs == str(tmp_path)
    with pytest.raises(SystemExit):
        b.parse(["--steps", "0"])
    small = np.arange(2 * 4 * 4 * 3, dtype=np.float64).reshape(2, 4, 4, 3)
    b.dump_outputs(tmp_path / "small", {"images": small})
    got = np.load(tmp_path / "small" / "images.npy")
    assert got.dtype == np.float32 and np.array_equal(got, small)
    big = np.arange(1024 * 64 * 64 * 3, dtype=np.float32).reshape(1024, 64, 64, 3)      # 50 MB x 2
    for d in ("a", "b"):
        b.dump_outputs(tmp_path / d, {"images": big, "other": big})
    files = sorted((tmp_path / "a").glob("*.npy"))
    assert [f.name for f in files] == ["images.npy", "other.npy"] and sum(f.stat().st_size for f in files) <= 64 * 10**6
    a0, b0 = np.load(tmp_path / "a" / "images.npy"), np.load(tmp_path / "b" / "images.npy")
    assert np.array_equal(a0, b0) and a0.shape[1:] == big.shape[1:] and a0.shape[0] > 500
    assert np.isin(a0[:, 0, 0, 0], big[:, 0, 0, 0]).all()                                # whole images of the output


def test_documents_quote_the_committed_profiles():
    """README.md and DESIGN.md carry ONE generated performance block (tools/perf_tables.py: the driver's BENCH_rNN.json records + the newest
    profiles/rNN collection); it must be what the files say (no number in the documents that a file under profiles/ contradicts)."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, str(REPO / "tools" / "perf_tables.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_hand_counted_loads_of_the_output_head_are_never_touched_in_flight():
    """head_dec_kernel (embed_dim <= 512) issues its row quads and its share of the decoder weights as asm loads hipcc does not count and waits
    for them with hand-written s_waitcnt vmcnt(N).  tools/isa_audit_head.py compiles rowops.hip for gfx950 and proves on the ISA -- a forward
    dataflow over every instantiation's basic blocks -- that no instruction names a destination register between its load and the wait that
    covers it (a phi copy did, once: every early-exit probe value was wrong), that there are no spills or AGPR parks, and that the MFMAs start
    before the last wait.  Cross-compiles without a GPU."""
    import shutil
    import subprocess
    import sys
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    r = subprocess.run([sys.executable, str(REPO / "tools" / "isa_audit_head.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(": OK") == 32


def test_every_lds_dma_request_has_a_wait_state_behind_its_m0_write():
    """An LDS-DMA request takes its LDS destination from M0, and gfx950 needs one wait state between an SALU write of M0 and the request that
    reads it; hipcc pads the sites it emits itself but not the inside of an asm string (wave_prims.h lds_dma16s, which gemm.hip, rowlin.hip and
    attention.hip's weight ring call).  tools/isa_audit_lds_dma.py compiles every translation unit for gfx950 and checks each kernel's instruction stream (across
    labels and branches) for a request whose previous instruction writes M0.  Cross-compiles without a GPU."""
    import shutil
    import subprocess
    import sys
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    r = subprocess.run([sys.executable, str(REPO / "tools" / "isa_audit_lds_dma.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    total = re.search(r"total: (\d+) LDS-DMA instructions, (\d+) findings", r.stdout)
    assert total and int(total.group(1)) > 0 and total.group(2) == "0", r.stdout
    for kernel in ("gemm256_kernel", "rowlin768_kernel", "qkv_attention_kernel", "mlp_fused_kernel"):
        assert kernel in r.stdout, f"{kernel} issues no LDS-DMA any more: the audit no longer sees it"
