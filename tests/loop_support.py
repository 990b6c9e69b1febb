"""What the sampling-loop tests share (test_guidance, test_autoguidance, test_multistep, test_known_region, test_x0_threshold, test_pag,
test_gpu_parity): synthetic models on the engine, the side stream the loops run on, the noise a device loop draws at a step, the sampler's
command line and the error model of the bf16 engine."""
import numpy as np
import torch

from duodiff_amd.config import ModelParams
from duodiff_amd.weights import synthetic_state_dict

# bf16 engine vs the reference: the gate on rms(eps - ref) / sigma(ref) is an ERROR MODEL, not a fit to the last run.  Every block rounds
# ~6 GEMM operands to bf16 (norm1 rows, the attention output, norm2 rows, the GELU'd hidden rows, the long-skip copy, P of the attention
# core), each with relative rms 2^-9 / sqrt(3) (uniform rounding error of an 8-bit significand), and the roundings of the `depth` blocks
# add in quadrature on a residual stream of spread ~sigma:  model = 2^-9 / sqrt(3) * sqrt(6 depth)  =  4.8e-3 (depth 3) .. 9.9e-3 (13)
# .. 1.27e-2 (21).  Observed on MI355X (profiles/r05/parity_numbers.txt): 0.47 .. 0.96 of the model.  The bound is the model x 1.5, fixed.
EPS_RMS_MODEL_MARGIN = 1.5


def eps_rms_bound(depth):
    return EPS_RMS_MODEL_MARGIN * 2.0 ** -9 / np.sqrt(3.0) * np.sqrt(6.0 * depth)


def uvit(cfg, seed, precision, max_batch=None):
    """a UViT of synthetic weights on the GPU, and its ModelParams"""
    from duodiff_amd.uvit import UViT
    mp = ModelParams.from_dict(cfg)
    m = UViT(**mp.as_dict(), precision=precision, max_batch=max_batch)
    m.load_state_dict(synthetic_state_dict(mp, seed))
    return m.eval().to("cuda"), mp


def engine_pair(cfg_a, cfg_b, seeds, max_batch, precision="bf16"):
    """the engine models of two configs (shallow and full, or guide and main) and the second one's ModelParams"""
    m_a, _ = uvit(cfg_a, seeds[0], precision, max_batch)
    m_b, mp = uvit(cfg_b, seeds[1], precision, max_batch)
    return m_a.engine_model(max_batch), m_b.engine_model(max_batch), mp


def side_stream():
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    return s


def philox_z(em, like, k, seed, stream, y=None, t=500.0):
    """the z a device loop draws at Philox counter k: a one-step dd_sample_affine with the row (0, 0, 1) returns exactly 0 + 0 + 1 * z"""
    from duodiff_amd.engine import sample_affine_loop
    z = like.clone()
    with torch.cuda.stream(stream):
        sample_affine_loop(em.ctx, em, None, z, [t], [0.0], [0.0], [1.0], [1], y=y, seed=seed, counter_base=k, noise="philox",
                           use_graph=False, stream=stream)
    stream.synchronize()
    return z


def philox_z2(em, like, k, seed, stream, y=None):
    """the z2 of a step: a one-step region call with m = 1, x0 = 0, ka = 0, kb = 1 on the row (0, 0, 0) returns 1 * (0 + 1 * z2) + 0 * 0"""
    from duodiff_amd.engine import KnownRegion, sample_affine_region_loop
    z = like.clone()
    B, _, S, _ = like.shape
    reg = KnownRegion(torch.zeros_like(like), torch.ones(B, 1, S, S, device="cuda"), np.zeros(1, np.float32), np.ones(1, np.float32))
    with torch.cuda.stream(stream):
        sample_affine_region_loop(em.ctx, em, None, z, reg, [500.0], [0.0], [0.0], [0.0], [0], y=y, seed=seed, counter_base=k,
                                  noise="philox", use_graph=False, stream=stream)
    stream.synchronize()
    return z


def known_region(plan, x0, mask, k0=0, k1=None):
    from duodiff_amd import sampler
    from duodiff_amd.engine import KnownRegion
    ka, kb = sampler.known_rows(plan)
    return KnownRegion(x0, mask, ka[k0:k1], kb[k0:k1])


def cli_argv(config, *extra, par="predict_noise"):
    return ["--checkpoint_path", "/nonexistent.pth", "--batch_size", "2", "--parametrization", par,
            "--output_folder", "/tmp/unused", "--config_path", str(config), *extra]
