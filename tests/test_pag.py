"""Perturbed-attention guidance (PAG; Ahn et al. 2024): eps = eps + s (eps - eps_perturbed), eps_perturbed the same model on the same x_t
with the self-attention map of the chosen blocks replaced by the identity (attention(q, k, v) = v): dd_forward_perturbed, dd_sample_perturbed,
dd_sample_affine_perturbed, dd_sample_multistep_perturbed, the kernels v_identity_kernel<512 | 768 | 1024> and v_copy_kernel<T>
(csrc/attention.hip) behind them and the sampler options --pag_scale / --pag_layers / --pag_layers_first.

CPU tests: the command line, validate_pag's rejections, the ctypes binding.
GPU tests (marked), kernels, against float64 of the SAME bf16-rounded operands, per element:
  * dd_dev_v_identity, patch rows:  |out - ref| <= half a bf16 ulp of ref + 2^-16 (|h| . |Wv|^T + |bv|), tests/test_gemm_path.py's bound of a
    bf16 GEMM result with the rounding's own half ulp; the extra-token rows, which the kernel normalises itself from fp32 rows: the same
    + tests/test_row_kernels.py's bf16 LayerNorm bound (2^-8 |hx| + 2 x its fp32 bound) carried through |Wv|.  Canary rows and every row
    outside the images keep 0xFFFF, the patch rows of the residual stream (NaN on the device) are never read, an image's rows do not
    depend on its batch.
  * dd_dev_v_copy: bit-equal to V, finite although the pad rows of the device tensor hold NaN, canaries intact.
GPU tests, model: dd_forward_perturbed against the unchanged numpy oracle run twice (the second time with oracle.uvit_oracle.attention
patched to proj(v) for the masked blocks), combined in float64 -- fp32 max <= 1e-4, bf16 rms <= eps_rms_bound(depth) (1 + 2 s) sigma, the
project's own bounds -- on every attention path (fused attn.qkv + attention, the qkv GEMM, the block tail's qkv, fp32); then the loops
against their own building blocks bit for bit, chains, graph keys, stale workspace bytes, argument errors, the CLI.
"""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest
import torch

import kernel_support
from conftest import REPO, TINY
from duodiff_amd import _lib as L
from duodiff_amd.config import ModelParams, load_config
from duodiff_amd.weights import synthetic_state_dict
from kernel_support import FP32_REL, NAN16, P, bf16, from_bf16_bits, gate, ulp_bf16
from loop_support import KINDS, QA512, TAIL256, TINY_COND, celeba_pair, cli_argv, dev_flags, engine_pair, eps_rms_bound, first_rows, images
from loop_support import labels, run_first_steps, run_steps, side_stream, uvit
from test_row_kernels import ln_rows, ln_tolerances

gpu = pytest.mark.gpu

CONFIGS = REPO / "configs"
CELEBA = CONFIGS / "uvit_celeba.yaml"
CELEBA_3 = CONFIGS / "uvit_celeba_3.yaml"


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_cli_pag_options_and_defaults():
    from duodiff_amd import sampler
    cfg, cfg3 = load_config(CELEBA), load_config(CELEBA_3)
    a = sampler.get_args(cli_argv(CELEBA))
    assert a.pag_scale is None and a.pag_layers is None and a.pag_layers_first is None
    assert sampler.validate_pag(a, cfg) is None
    a = sampler.get_args(cli_argv(CELEBA, "--pag_scale", "3"))
    assert a.pag_scale == 3.0
    assert sampler.validate_pag(a, cfg) == (3.0, [6], [])                      # depth 13: mid = block 6
    a = sampler.get_args(cli_argv(CELEBA, "--pag_scale", "0"))
    assert a.pag_scale == 0.0 and a.pag_scale is not None                      # 0 selects the path too
    assert sampler.validate_pag(a, cfg)[0] == 0.0
    a = sampler.get_args(cli_argv(CELEBA, "--pag_scale", "1.5", "--pag_layers", "5", "mid", "7"))
    assert sampler.validate_pag(a, cfg) == (1.5, [5, 6, 7], [])
    # a pair: --pag_layers is the late model's, --pag_layers_first the first model's, both default to their own mid
    a = sampler.get_args(cli_argv(CELEBA_3, "--pag_scale", "2"))
    assert sampler.validate_pag(a, cfg3, cfg) == (2.0, [1], [6])
    a = sampler.get_args(cli_argv(CELEBA_3, "--pag_scale", "2", "--pag_layers", "0", "12", "--pag_layers_first", "2"))
    assert sampler.validate_pag(a, cfg3, cfg) == (2.0, [2], [0, 12])
    from duodiff_amd.engine import layer_mask
    assert layer_mask([0, 12]) == 0x1001 and layer_mask([]) == 0 and layer_mask(5) == 5
    with pytest.raises(ValueError):
        layer_mask([32])


@pytest.mark.parametrize("config,extra,match", [
    ("uvit_celeba.yaml", ["--pag_scale", "1", "--pag_layers", "13"], "outside"),                 # depth 13: blocks 0 .. 12
    ("uvit_celeba.yaml", ["--pag_scale", "1", "--pag_layers", "-1"], "outside"),
    ("uvit_celeba.yaml", ["--pag_scale", "1", "--pag_layers", "middle"], "mid"),
    ("uvit_celeba.yaml", ["--pag_scale", "nan"], "finite"),
    ("uvit_celeba.yaml", ["--pag_scale", "inf"], "finite"),
    ("uvit_celeba.yaml", ["--pag_layers", "3"], "pag_scale"),
    ("uvit_celeba.yaml", ["--pag_scale", "1", "--pag_layers_first", "1"], "pair"),
    ("uvit_imagenet256.yaml", ["--pag_scale", "1", "--cfg_scale", "0.4", "--class_label", "3"], "exclusive"),
    ("uvit_celeba.yaml", ["--pag_scale", "1", "--known_image", "k.npy", "--known_mask", "m.npy"], "exclusive"),
    ("uvit_celeba.yaml", ["--pag_scale", "1", "--init_image", "i.npy", "--strength", "0.5"], "exclusive"),
    ("uvit_celeba.yaml", ["--pag_scale", "1", "--clip_x0"], "exclusive"),
    ("uvit_celeba.yaml", ["--pag_scale", "1", "--dynamic_threshold", "0.995"], "exclusive"),
])
def test_validate_pag_rejects_before_any_gpu_work(config, extra, match):
    """validate_pag against the YAML alone: no model is built, no GPU is touched (this runs on the CPU box)."""
    from duodiff_amd import sampler
    args = sampler.get_args(cli_argv(CONFIGS / config, *extra))
    with pytest.raises(ValueError, match=match):
        sampler.validate_pag(args, load_config(CONFIGS / config))


@pytest.mark.parametrize("extra,match", [
    (["--pag_scale", "1", "--autoguidance_scale", "1.0"], "exclusive"),
    (["--pag_scale", "1", "--pag_layers_first", "3"], "outside"),                                # the first model has 3 blocks
    (["--pag_scale", "1", "--pag_layers", "13"], "outside"),
])
def test_validate_pag_rejects_a_pair(extra, match):
    from duodiff_amd import sampler
    args = sampler.get_args(cli_argv(CELEBA_3, "--checkpoint_path_late", "/nonexistent.pth", "--config_path_late", str(CELEBA), *extra))
    with pytest.raises(ValueError, match=match):
        sampler.validate_pag(args, load_config(CELEBA_3), load_config(CELEBA))


def test_cli_main_rejects_pag_options_before_it_builds_a_model(tmp_path):
    from duodiff_amd import sampler
    argv = cli_argv(CELEBA, "--pag_scale", "1", "--pag_layers", "13")
    argv[argv.index("--output_folder") + 1] = str(tmp_path / "out")
    with pytest.raises(ValueError, match="outside"):
        sampler.main(argv)


def test_eesampler_does_not_take_the_options():
    from duodiff_amd import eesampler
    src = (REPO / "duodiff_amd" / "eesampler.py").read_text()
    assert "pag" not in src and hasattr(eesampler, "main")


def test_lib_binds_the_perturbed_entry_points():
    assert L.ABI_VERSION == 6
    assert C.sizeof(L.dd_pag) == 12
    p = L.dd_pag(0.4, 0x1001, 2)
    assert abs(p.scale - 0.4) < 1e-7 and p.layers_first == 0x1001 and p.layers_late == 2
    assert L.SIGNATURES["dd_forward_perturbed"][1] == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.POINTER(L.dd_pag),
                                                       C.c_void_p, C.c_int, C.c_void_p]
    assert L.SIGNATURES["dd_sample_perturbed"][1] == [C.c_void_p, C.POINTER(L.dd_sample_args), C.POINTER(L.dd_pag), C.c_void_p]
    assert L.SIGNATURES["dd_sample_affine_perturbed"][1] == [C.c_void_p, C.POINTER(L.dd_affine_sample_args), C.POINTER(L.dd_pag), C.c_void_p]
    assert L.SIGNATURES["dd_sample_multistep_perturbed"][1] == [C.c_void_p, C.POINTER(L.dd_multistep_sample_args), C.POINTER(L.dd_pag),
                                                                C.c_void_p]
    assert L.SIGNATURES["dd_dev_v_identity"][1] == L.SIGNATURES["dd_dev_qkv_attention_rows"][1]
    lib = L.load()
    assert lib.dd_abi_version() == 6
    for name in ("dd_forward_perturbed", "dd_sample_perturbed", "dd_sample_affine_perturbed", "dd_sample_multistep_perturbed",
                 "dd_dev_v_identity", "dd_dev_v_copy"):
        assert hasattr(lib, name)


def test_the_kernel_gates_reject_a_wrong_v():
    """The elementwise gate of the v_identity tests on the CPU: bf16(float64 result) passes; the k block taken for the v block, a row
    shifted by one, and a dropped bias do not."""
    r = np.random.default_rng(5)
    D = 512
    h = bf16(r.standard_normal((64, D), dtype=np.float32))
    w = bf16((r.standard_normal((3 * D, D)) / np.sqrt(D)).astype(np.float32))
    b = (0.3 * r.standard_normal(3 * D)).astype(np.float32)
    ref, tol = _v_ref(h, w, b, D)
    assert gate(bf16(ref.astype(np.float32)), ref, tol, "bf16 of the reference") <= 1.0
    wrong_k = h.astype(np.float64) @ w[D:2 * D].astype(np.float64).T + b[D:2 * D]
    for what, bad in (("k for v", wrong_k), ("row shift", np.roll(ref, 1, 0)), ("no bias", ref - b[2 * D:])):
        with pytest.raises(AssertionError):
            gate(bf16(bad.astype(np.float32)), ref, tol, what)


# ---- GPU, kernels -----------------------------------------------------------------------------------------------------------
def _v_ref(h, w, bias, D):
    """float64 v = h . Wv^T + bv of operands that are already bf16 values, and the bound of its bf16 result: half an ulp + 2^-16 of the sum
    of magnitudes"""
    h64, wv = h.astype(np.float64), w[2 * D:].astype(np.float64)
    bv = bias[2 * D:].astype(np.float64) if bias is not None else np.zeros(D)
    ref = h64 @ wv.T + bv
    tol = 0.5 * ulp_bf16(ref) + FP32_REL * (np.abs(h64) @ np.abs(wv).T + np.abs(bv)) + 1e-30
    return ref, tol


def _v_case(D, B, E, with_bias, seed, offset=0.0):
    """h [B L, D] and wqkv [3 D, D] as bf16 values, bias [3 D] or None, xres [B L, D] fp32 (the extra-token rows at `offset` sigma; its
    patch rows are never used), ln [2, D]"""
    L_ = 256 + E
    r = np.random.default_rng(seed)
    h = bf16(r.standard_normal((B * L_, D), dtype=np.float32))
    w = bf16((r.standard_normal((3 * D, D)) / np.sqrt(D)).astype(np.float32))
    bias = (0.3 * r.standard_normal(3 * D)).astype(np.float32) if with_bias else None
    xe, g, b = ln_rows(B * E, D, offset, 1.0, seed + 1)
    xres = r.standard_normal((B, L_, D)).astype(np.float32)
    xres[:, :E] = xe.reshape(B, E, D)
    return h, w, bias, xres.reshape(B * L_, D), np.ascontiguousarray(np.stack([g, b]), np.float32)


def _run_v_identity(B, E, H, h, w, bias, xres, ln):
    ctx = kernel_support.ctx()
    D, L_ = 64 * H, 256 + E
    out = np.full((B * L_ + 8, D), 0xA5A5, np.uint16)
    st = ctx.lib.dd_dev_v_identity(ctx.handle, B, L_, H, E, P(h), P(w), P(bias), P(xres), P(ln), P(out), 0, None, C.byref(C.c_float(0)))
    return st, out


def _check_v_identity(D, B, E, with_bias, seed, offset=0.0):
    H, L_ = D // 64, 256 + E
    h, w, bias, xres, ln = _v_case(D, B, E, with_bias, seed, offset)
    st, out = _run_v_identity(B, E, H, h, w, bias, xres, ln)
    assert st == L.DD_OK, kernel_support.ctx().lib.dd_last_error(kernel_support.ctx().handle).decode()
    assert (out[B * L_:] == NAN16).all(), "canary rows behind the output were written"
    got = from_bf16_bits(out[:B * L_]).astype(np.float64)
    assert np.isfinite(got).all(), "a row the kernel must not read (NaN on the device) reached the output"
    tok = np.arange(B * L_) % L_
    patch, extra = tok >= E, tok < E
    ref, tol = _v_ref(h, w, bias, D)
    rp = gate(got[patch], ref[patch], tol[patch], f"v_identity D={D} B={B} E={E}: patch rows")
    # the extra-token rows: norm1 of the fp32 rows in float64 (not rounded), the kernel's bf16 rounding of it inside the LayerNorm bound
    x_many = ln_rows(516, D, offset, 1.0, seed + 2)[0]
    hx, _, t16 = ln_tolerances(xres[extra], ln[0], ln[1], x_many)
    wv = w[2 * D:].astype(np.float64)
    bv = bias[2 * D:].astype(np.float64) if with_bias else np.zeros(D)
    ref_e = hx @ wv.T + bv
    tol_e = 0.5 * ulp_bf16(ref_e) + FP32_REL * (np.abs(hx) @ np.abs(wv).T + np.abs(bv)) + t16 @ np.abs(wv).T
    re = gate(got[extra], ref_e, tol_e, f"v_identity D={D} B={B} E={E}: extra-token rows")
    print(f"v_identity D={D} B={B} E={E} bias={with_bias} offset={offset}: max err/bound {rp:.3f} (patch rows), {re:.3f} (extra-token rows)")
    return out


@gpu
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("B,E", [(1, 1), (3, 2), (5, 1)])
@pytest.mark.parametrize("D", [512, 768, 1024])
def test_v_identity_against_float64_reference(D, B, E, with_bias):
    _check_v_identity(D, B, E, with_bias, seed=1000 + D + 10 * B + E)


@gpu
def test_v_identity_extra_rows_at_an_offset_of_100_sigma():
    """the extra-token rows of the residual stream sit at 100 sigma: a one-pass variance in the in-kernel norm1 loses them"""
    _check_v_identity(768, 3, 2, True, seed=77, offset=100.0)


@gpu
def test_v_identity_an_image_does_not_depend_on_its_batch():
    D, E, H = 512, 2, 8
    L_ = 256 + E
    h, w, bias, xres, ln = _v_case(D, 3, E, True, 31)
    st3, out3 = _run_v_identity(3, E, H, h, w, bias, xres, ln)
    assert st3 == L.DD_OK
    for b in range(3):
        sl = slice(b * L_, (b + 1) * L_)
        st1, out1 = _run_v_identity(1, E, H, np.ascontiguousarray(h[sl]), w, bias, np.ascontiguousarray(xres[sl]), ln)
        assert st1 == L.DD_OK and (out1[L_:] == NAN16).all()
        assert np.array_equal(out1[:L_], out3[sl]), f"image {b} of B = 3 differs from its B = 1 call"


@gpu
def test_v_identity_refuses_what_it_does_not_support():
    ctx = kernel_support.ctx()
    h, w, bias, xres, ln = _v_case(512, 1, 1, False, 3)
    for B, L_, H, E in ((1, 257, 4, 1), (1, 256, 8, 1), (1, 259, 8, 3), (1, 258, 8, 1)):
        out = np.full((B * L_ + 8, 64 * H), 0xA5A5, np.uint16)
        st = ctx.lib.dd_dev_v_identity(ctx.handle, B, L_, H, E, P(h), P(w), None, P(xres), P(ln), P(out), 0, None, C.byref(C.c_float(0)))
        assert st == L.DD_ERR_UNSUPPORTED and (out == 0xA5A5).all()
    out = np.full((257 + 8, 512), 0xA5A5, np.uint16)
    st = ctx.lib.dd_dev_v_identity(ctx.handle, 1, 257, 8, 1, P(h), P(w), None, None, None, P(out), 0, None, C.byref(C.c_float(0)))
    assert st == L.DD_ERR_INVALID and (out == 0xA5A5).all()          # the hx mode does not exist here


@gpu
@pytest.mark.parametrize("B,H", [(3, 1), (2, 8)])
@pytest.mark.parametrize("L_", [17, 18, 257, 258])
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_v_copy_is_bit_equal_to_v(prec, L_, B, H):
    ctx = kernel_support.ctx()
    D = 64 * H
    r = np.random.default_rng(7 * L_ + B + H)
    qkv = r.standard_normal((B, 3, H, L_, 64), dtype=np.float32)
    if prec == "bf16":
        qkv = bf16(qkv)
    out = np.full((B * L_ + 8, D), 0xA5A5 if prec == "bf16" else 0xA5A5A5A5, np.uint16 if prec == "bf16" else np.uint32)
    st = ctx.lib.dd_dev_v_copy(ctx.handle, 0 if prec == "bf16" else 1, B, L_, H, P(qkv), P(out), 0, None, C.byref(C.c_float(0)))
    assert st == L.DD_OK, ctx.lib.dd_last_error(ctx.handle).decode()
    assert (out[B * L_:] == (NAN16 if prec == "bf16" else 0xFFFFFFFF)).all(), "canary rows behind the output were written"
    v = qkv[:, 2].transpose(0, 2, 1, 3).reshape(B * L_, D)                    # "B H L D -> B L (H D)"
    want = (v.view(np.uint32) >> 16).astype(np.uint16) if prec == "bf16" else v.view(np.uint32)
    got = out[:B * L_]
    vals = from_bf16_bits(got) if prec == "bf16" else got.view(np.float32)
    assert np.isfinite(vals).all(), "a pad row of the qkv tensor (NaN on the device) reached the output"
    assert np.array_equal(got, want)


@gpu
def test_v_copy_refuses_a_long_sequence():
    ctx = kernel_support.ctx()
    qkv = np.zeros((1, 3, 1, 289, 64), np.float32)
    out = np.full((289 + 8, 64), 0xA5A5, np.uint16)
    st = ctx.lib.dd_dev_v_copy(ctx.handle, 0, 1, 289, 1, P(qkv), P(out), 0, None, C.byref(C.c_float(0)))
    assert st == L.DD_ERR_UNSUPPORTED and (out == 0xA5A5).all()


# ---- GPU, model -------------------------------------------------------------------------------------------------------------
FORWARD_CASES = {
    "tiny": (TINY, 5, 0), "tiny_classes": (TINY_COND, 5, 0), "qa512": (QA512, 2, 0), "qa512_no_fused_qa": (QA512, 2, L.DD_DEV_NO_FUSED_QA),
    "tail256": (TAIL256, 3, 0),
}


def _block_prefixes(depth):
    half = depth // 2
    return [f"in_blocks.{i}." for i in range(half)] + ["mid_block."] + [f"out_blocks.{i}." for i in range(half)]


def _oracle_pair(monkeypatch, cfg, sd, x, t, y, layers):
    """(eps, eps_perturbed) of the numpy oracle in float64: the second run with oracle.uvit_oracle.attention replaced by proj(v) for the
    blocks `layers` (forward order)"""
    import oracle
    from oracle import uvit_oracle as uo
    mp = ModelParams.from_dict(cfg)
    orc = oracle.UViTOracle(mp.as_dict(), {k: v.numpy() for k, v in sd.items()})
    tv = np.full((x.shape[0],), t, np.float32)
    plain = orc(x, tv, y).astype(np.float64)
    masked = {_block_prefixes(mp.depth)[i] + "attn." for i in layers}
    real = uo.attention

    def attention(xx, p, prefix, num_heads):
        if prefix not in masked:
            return real(xx, p, prefix, num_heads)
        Cdim = xx.shape[-1]
        qkv = uo.linear(xx, p[prefix + "qkv.weight"], p.get(prefix + "qkv.bias"))      # "B L (K H D)": v = the last third, heads merged
        return uo.linear(qkv[..., 2 * Cdim:], p[prefix + "proj.weight"], p[prefix + "proj.bias"])

    with monkeypatch.context() as mpatch:
        mpatch.setattr(uo, "attention", attention)
        pert = orc(x, tv, y).astype(np.float64)
    return plain, pert


@gpu
@pytest.mark.parametrize("mask", ["mid", "all"])
@pytest.mark.parametrize("case", sorted(FORWARD_CASES))
def test_forward_perturbed_vs_oracle(monkeypatch, case, mask):
    cfg, B, flags = FORWARD_CASES[case]
    mp = ModelParams.from_dict(cfg)
    layers = [mp.depth // 2] if mask == "mid" else list(range(mp.depth))
    s, t = 0.4, 611.0
    sd = synthetic_state_dict(mp, 61)
    g = torch.Generator().manual_seed(62)
    x = torch.randn(B, mp.in_chans, mp.img_size, mp.img_size, generator=g)
    y = torch.randint(0, 11, (B,), generator=g) if mp.num_classes > 0 else None
    plain, pert = _oracle_pair(monkeypatch, cfg, sd, x.numpy(), t, None if y is None else y.numpy(), layers)
    want = plain + s * (plain - pert)
    sigma = float(plain.std())
    moved = float(np.sqrt(((pert - plain) ** 2).mean())) / sigma
    assert moved >= 0.05, "the oracle's own perturbation is too small to test anything"
    for prec in ("fp32", "bf16"):
        m, _ = uvit(cfg, 61, prec, max_batch=2 * B)
        with dev_flags(kernel_support.ctx(), flags):
            em = m.engine_model(2 * B)
        yd = None if y is None else y.cuda()
        got = em.forward_perturbed(x.cuda(), t, yd, s, layers).cpu().numpy().astype(np.float64)
        base = em.forward(x.cuda(), t, yd).cpu().numpy().astype(np.float64)
        torch.cuda.synchronize()
        assert np.isfinite(got).all()
        err, rms = float(np.abs(got - want).max()), float(np.sqrt(((got - want) ** 2).mean()))
        own = float(np.sqrt(((got - base) ** 2).mean())) / (s * sigma)           # rms(eps - eps_perturbed) / sigma of the engine itself
        print(f"{case} {mask} {prec}: perturbed eps vs oracle max {err:.3e} rms {rms:.3e} (sigma {sigma:.3f}); the perturbation moves eps by "
              f"{moved:.3f} sigma rms (oracle), {own:.3f} (engine)")
        assert own >= 0.05, "the engine's perturbed pass equals its plain pass: nothing was perturbed"
        if prec == "fp32":
            assert err <= 1e-4
        else:
            assert rms <= eps_rms_bound(mp.depth) * (1 + 2 * s) * sigma
        del em, m


@gpu
@pytest.mark.parametrize("case", ["tiny", "tiny_classes", "qa512", "tail256"])
def test_mask_zero_equals_dd_forward(case):
    """mask 0: both halves of the 2 B rows are the plain forward, d is exactly 0 and any scale gives the bits of dd_forward"""
    cfg, B, _ = FORWARD_CASES[case]
    mp = ModelParams.from_dict(cfg)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, mp.in_chans, mp.img_size, mp.img_size, generator=g).cuda()
    y = torch.randint(0, 11, (B,), generator=g).cuda() if mp.num_classes > 0 else None
    for prec in ("bf16", "fp32"):
        m, _ = uvit(cfg, 63, prec, max_batch=2 * B)
        em = m.engine_model(2 * B)
        base = em.forward(x, 400.0, y)
        for s in (0.0, 1.7, -3.0):
            assert torch.equal(em.forward_perturbed(x, 400.0, y, s, 0), base), f"{case} {prec}: mask 0 at scale {s} differs from dd_forward"
        assert torch.isfinite(base).all()
        del em, m


def _tiny_pair(seeds=(41, 42), max_batch=12):
    return engine_pair(dict(TINY, depth=1), dict(TINY, depth=3), seeds, max_batch)[:2]


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", ["tiny_forced", "celeba_default"])
def test_scale_zero_equals_the_unguided_loop(case, kind):
    """scale 0 with a full mask, Philox noise, the backbone switch inside: dd_sample_perturbed / _affine_ / _multistep_ == the unguided
    loops bit for bit (eps + 0 d; the first half of the 2 B rows is the unguided forward, the Philox ids are the unguided loop's)"""
    from duodiff_amd.engine import Perturbed
    if case == "tiny_forced":
        B, S, n, sw, flags = 6, 8, 8, 3, L.DD_DEV_FORCE_CHAINS
        es, ef = _tiny_pair(max_batch=2 * B)
        full = Perturbed(0.0, [0], [0, 1, 2])
    else:
        B, S, n, sw, flags = 32, 64, 3, 1, 0
        es, ef = celeba_pair(2 * B)[:2]
        full = Perturbed(0.0, [0, 1, 2], list(range(13)))
    ctx, x0, stream = es.ctx, images(B, 3, S, 7), side_stream()
    outs = {}
    for name, guidance in (("unguided", None), ("scale0", full)):
        outs[name] = (run_first_steps(kind, es, ef, x0, stream, switch=sw, n=n, seed=21, noise="philox", flags=flags, guidance=guidance),
                      ctx.lib.dd_dev_last_sample_chains(ctx.handle))
    assert outs["unguided"][1] == outs["scale0"][1] == 2
    assert torch.isfinite(outs["scale0"][0]).all()
    assert torch.equal(outs["scale0"][0], outs["unguided"][0]), "scale 0 differs from the unguided loop"


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_perturbed_loops_equal_manual_steps(kind):
    """No noise, s = 1.7, the backbone switch inside, each model with its own mask: the device loop, graph-replayed and eager,
    == forward_perturbed + ddpm_step / affine_step / multistep_step per step"""
    from duodiff_amd.engine import Perturbed
    B, s, n, sw = 4, 1.7, 8, 3
    es, ef = _tiny_pair(max_batch=2 * B)
    x0, stream = images(B, 3, 8, 11), side_stream()
    pag = Perturbed(s, [0], [1, 2])
    loops = [run_first_steps(kind, es, ef, x0, stream, switch=sw, n=n, noise="none", use_graph=ug, guidance=pag) for ug in (True, False)]
    plain = run_first_steps(kind, es, ef, x0, stream, switch=sw, n=n, noise="none", guidance=None)
    xm, h = run_steps(kind, es, x0, first_rows(kind, n), stream, late=ef, switch_after=sw, noise="none", guidance=pag)
    manual = xm if kind != "multistep" else torch.stack([xm, h])
    assert torch.isfinite(manual).all() and not torch.equal(xm, x0)
    assert torch.equal(loops[0], loops[1]), "graph replay differs from eager launches"
    assert torch.equal(loops[0], manual), "the perturbed loop differs from its manual steps"
    assert not torch.equal(loops[0], plain), "the perturbed loop equals the unguided loop: nothing was guided"


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_perturbed_two_chains_equal_one_chain(kind):
    """s = 0.4, Philox noise, the switch inside, B = 6: the two image-split chains == DD_DEV_NO_CHAINS bit for bit"""
    from duodiff_amd.engine import Perturbed
    B = 6
    es, ef = _tiny_pair(max_batch=2 * B)
    ctx, x0, stream = es.ctx, images(B, 3, 8, 13), side_stream()
    pag = Perturbed(0.4, [0], [1])
    outs = {}
    for name, flags in (("chained", L.DD_DEV_FORCE_CHAINS), ("single", L.DD_DEV_NO_CHAINS)):
        outs[name] = (run_first_steps(kind, es, ef, x0, stream, switch=3, n=8, seed=23, noise="philox", flags=flags, guidance=pag),
                      ctx.lib.dd_dev_last_sample_chains(ctx.handle))
    assert outs["chained"][1] == 2 and outs["single"][1] == 1
    assert torch.isfinite(outs["single"][0]).all()
    assert torch.equal(outs["chained"][0], outs["single"][0]), "perturbed chains differ from the single chain"


@gpu
def test_a_new_mask_or_scale_is_not_a_stale_graph():
    """Calls with (scale, first mask, late mask) changing one at a time on the same models: each equals a run of freshly built models"""
    from duodiff_amd.engine import Perturbed
    B = 4
    x0, stream = images(B, 3, 8, 15), side_stream()
    settings = [Perturbed(0.4, [0], [1]), Perturbed(1.0, [0], [1]), Perturbed(1.0, [0], [2]), Perturbed(1.0, [], [2]), Perturbed(0.4, [0], [1])]

    def run(es, ef, pag):
        return run_first_steps("ddpm", es, ef, x0, stream, switch=3, n=8, seed=25, noise="philox", guidance=pag)

    es, ef = _tiny_pair(max_batch=2 * B)
    got = [run(es, ef, p) for p in settings]
    fresh = []
    for p in settings[:4]:
        fs, ff = _tiny_pair(max_batch=2 * B)
        fresh.append(run(fs, ff, p))
        del fs, ff
    fresh.append(fresh[0])
    for i in range(3):
        assert not torch.equal(fresh[i], fresh[i + 1])
    for p, g, f in zip(settings, got, fresh):
        assert torch.equal(g, f), f"{p}: replayed a graph of another setting"


@gpu
def test_perturbed_loop_reads_no_stale_workspace_bytes():
    """One forced-chains case with both chains' workspaces poisoned (NaN bytes) before the call == the same case on fresh models, on the
    path that reads the qkv tensor (tiny) and on the one that reads norm1 in fragment order (embed_dim 512)"""
    from duodiff_amd.engine import Perturbed
    for cfg_s, cfg_f, B, S, n in ((dict(TINY, depth=1), dict(TINY, depth=3), 6, 8, 6), (dict(QA512, depth=1), QA512, 2, 64, 2)):
        x0, stream = images(B, 3, S, 17), side_stream()
        outs = []
        for poison in (False, True):
            es, ef, _ = engine_pair(cfg_s, cfg_f, (71, 72), 2 * B)
            ctx = es.ctx
            if poison:
                with torch.cuda.stream(stream):
                    for e in (es, ef):
                        ctx.check(ctx.lib.dd_dev_poison_workspaces(ctx.handle, e.handle, stream.cuda_stream))
            outs.append((run_first_steps("ddpm", es, ef, x0, stream, switch=1, n=n, seed=27, noise="philox", flags=L.DD_DEV_FORCE_CHAINS,
                                         guidance=Perturbed(0.4, [0], [1, 2])), ctx.lib.dd_dev_last_sample_chains(ctx.handle)))
            del es, ef
        assert outs[0][1] == outs[1][1] == 2
        assert torch.isfinite(outs[0][0]).all() and not torch.equal(outs[0][0], x0)
        assert torch.equal(outs[0][0], outs[1][0]), "the perturbed loop differs after the workspaces were poisoned"


@gpu
def test_invalid_perturbed_calls_are_rejected_before_anything_is_enqueued():
    """DD_ERR_INVALID with a message, the tensors untouched and no graph captured: a null struct, a non-finite scale, a mask bit at or
    above the depth (of either model), 2 B > max_batch, an early-exit model, missing / superfluous labels"""
    from duodiff_amd.engine import Model
    B = 4
    es, ef = _tiny_pair(max_batch=2 * B)                        # depths 1 and 3
    ctx, lib = es.ctx, es.ctx.lib
    small, _ = uvit(dict(TINY, depth=1), 81, "bf16", max_batch=B)          # room for B rows only
    es_small = small.engine_model(B)
    cond, _ = uvit(dict(TINY_COND, depth=1), 82, "bf16", 2 * B)
    ec = cond.engine_model(2 * B)
    ee = Model(ctx, ModelParams.from_dict(TINY), 2 * B)
    ee.enable_early_exit("mlp_probe_per_layer")
    x0 = images(B, 3, 8, 19)
    y = labels(B, 10, 20)
    stream = side_stream()
    # (first, late, (scale, first mask, late mask) or None, labels, message)
    cases = [(es, None, None, None, "null dd_pag"), (es, None, (float("inf"), 1, 0), None, "finite"), (es, None, (float("nan"), 1, 0), None, "finite"),
             (es, None, (0.4, 2, 0), None, "depth"), (es, ef, (0.4, 1, 8), None, "depth"), (es_small, None, (0.4, 1, 0), None, "max_batch"),
             (ee, None, (0.4, 1, 0), None, "early-exit"), (ec, None, (0.4, 1, 0), None, "without labels"), (es, None, (0.4, 1, 0), y, "with labels")]
    n0 = lib.dd_dev_graph_captures(ctx.handle)
    for first, late, p, given, msg in cases:
        ps = L.dd_pag(*p) if p else None
        pref = C.byref(ps) if ps else None
        yp = given.data_ptr() if given is not None else None
        for entry in ("sample", "affine", "multistep") if late else ("forward", "sample", "affine", "multistep"):
            x, eps, h = x0.clone(), torch.zeros_like(x0), torch.zeros_like(x0)
            with torch.cuda.stream(stream):
                if entry == "forward":
                    rc = lib.dd_forward_perturbed(ctx.handle, first.handle, C.c_void_p(x.data_ptr()), 500.0, C.c_void_p(yp), pref,
                                                  C.c_void_p(eps.data_ptr()), B, C.c_void_p(stream.cuda_stream))
                elif entry == "sample":
                    a = L.dd_sample_args()
                    a.first, a.late, a.t_switch, a.t_start, a.t_end = first.handle, late.handle if late else None, 3, 999, 995
                    a.noise_mode, a.use_graph, a.seed, a.y_dev, a.x_dev, a.B = L.DD_NOISE_PHILOX, 1, 1, yp, x.data_ptr(), B
                    rc = lib.dd_sample_perturbed(ctx.handle, C.byref(a), pref, C.c_void_p(stream.cuda_stream))
                else:
                    n = 3
                    f = (C.c_float * n)(900.0, 600.0, 300.0)
                    one = (C.c_float * n)(1.0, 1.0, 1.0)
                    nz = (C.c_int32 * n)(0, 0, 0)
                    a = L.dd_affine_sample_args() if entry == "affine" else L.dd_multistep_sample_args()
                    a.first, a.late, a.n_steps, a.switch_after = first.handle, late.handle if late else None, n, 1
                    a.t, a.a, a.b, a.c, a.noise = f, one, one, one, nz
                    a.noise_mode, a.use_graph, a.seed, a.y_dev, a.x_dev, a.B = L.DD_NOISE_NONE, 1, 1, yp, x.data_ptr(), B
                    if entry == "affine":
                        rc = lib.dd_sample_affine_perturbed(ctx.handle, C.byref(a), pref, C.c_void_p(stream.cuda_stream))
                    else:
                        a.d, a.p, a.q, a.hist, a.h_dev = one, one, one, nz, h.data_ptr()
                        rc = lib.dd_sample_multistep_perturbed(ctx.handle, C.byref(a), pref, C.c_void_p(stream.cuda_stream))
            stream.synchronize()
            assert rc == L.DD_ERR_INVALID, f"{entry} {msg}: status {rc}"
            assert msg in lib.dd_last_error(ctx.handle).decode(), lib.dd_last_error(ctx.handle).decode()
            assert torch.equal(x, x0) and not eps.any() and not h.any(), f"{entry} {msg}: something was enqueued"
    # one model as first and late with two different masks: one captured graph per model could not serve both
    x = x0.clone()
    a = L.dd_sample_args()
    a.first, a.late, a.t_switch, a.t_start, a.t_end = ef.handle, ef.handle, 3, 999, 995
    a.noise_mode, a.use_graph, a.seed, a.y_dev, a.x_dev, a.B = L.DD_NOISE_PHILOX, 1, 1, None, x.data_ptr(), B
    ps = L.dd_pag(0.4, 1, 2)
    assert lib.dd_sample_perturbed(ctx.handle, C.byref(a), C.byref(ps), C.c_void_p(stream.cuda_stream)) == L.DD_ERR_INVALID
    assert "one model" in lib.dd_last_error(ctx.handle).decode() and torch.equal(x, x0)
    assert lib.dd_dev_graph_captures(ctx.handle) == n0
    with pytest.raises(ValueError):
        es.forward_perturbed(x0, 500.0, None, 0.4, [1])


@gpu
def test_get_samples_with_pag_runs_every_sampler():
    """get_samples(pag=...) through the one step plan: DDPM (cut short), DDIM and DPM-Solver++ on a pair, device noise and the step-by-step
    torch_cpu path; scale 0 equals the run without the option (device noise), a scale moves the samples"""
    from duodiff_amd import sampler
    ms, _ = uvit(dict(TINY, depth=1), 91, "bf16", None)
    mf, _ = uvit(dict(TINY, depth=3), 92, "bf16", None)
    common = dict(batch_size=3, postprocessing=sampler.predict_noise_postprocessing, seed=3, num_channels=3, sample_height=8, sample_width=8,
                  late_model=mf, t_switch=4)
    for kw in (dict(num_steps=8), dict(use_ddim=True, ddim_steps=6), dict(solver="dpmsolver++", solver_steps=6)):
        for noise in ("device", "torch_cpu"):
            base, _ = sampler.get_samples(ms, noise=noise, **common, **kw)
            zero, _ = sampler.get_samples(ms, noise=noise, pag=(0.0, [0], [0, 1, 2]), **common, **kw)
            moved, _ = sampler.get_samples(ms, noise=noise, pag=(2.0, [0], [1]), **common, **kw)
            assert np.isfinite(moved).all() and moved.shape == (3, 8, 8, 3)
            assert np.array_equal(zero, base), f"{kw} {noise}: scale 0 differs from the run without the option"
            assert not np.array_equal(moved, base), f"{kw} {noise}: the option changed nothing"
    with pytest.raises(ValueError, match="depth"):
        sampler.get_samples(ms, pag=(1.0, [1], [0]), **common)
    with pytest.raises(ValueError, match="combine"):
        sampler.get_samples(ms, pag=(1.0, [0], [0]), cfg_scale=0.4, **common)


@gpu
def test_cli_pag_end_to_end(tmp_path):
    """A synthetic unconditional checkpoint written here: --pag_scale 2 writes finite samples of the right shape, which differ from the
    --pag_scale 0 run, which equals the run without the option"""
    import yaml
    cfg = dict(TINY, depth=3, img_size=16)
    (tmp_path / "m.yaml").write_text(yaml.safe_dump({"model_params": cfg}))
    torch.save(dict(synthetic_state_dict(ModelParams.from_dict(cfg), 91)), tmp_path / "m.pth")
    got = {}
    for name, extra in (("2", ["--pag_scale", "2", "--pag_layers", "mid", "2"]), ("0", ["--pag_scale", "0"]), ("off", [])):
        out = tmp_path / f"out{name}"
        cmd = [sys.executable, "-m", "duodiff_amd.sampler", "--seed", "5", "--checkpoint_path", str(tmp_path / "m.pth"),
               "--config_path", str(tmp_path / "m.yaml"), "--batch_size", "3", "--parametrization", "predict_noise",
               "--output_folder", str(out), "--no_png", "--use_ddim", "--ddim_steps", "10", *extra]
        r = subprocess.run(cmd, cwd=str(REPO), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        got[name] = np.load(out / "samples.npy")
        assert got[name].shape == (3, 16, 16, 3) and np.isfinite(got[name]).all()
    assert not np.array_equal(got["2"], got["0"])
    assert np.array_equal(got["0"], got["off"])
