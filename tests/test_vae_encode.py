"""KL-VAE encode: FrozenAutoencoderKL.encode_moments / sample / encode of the reference
(models/utils/autoencoder.py:203-317, 468-484) on the engine (dd_vae_encode / dd_vae_sample), the Python mirror and the sampler's
--encode_images, pinned by the reference-generated fixture tests/golden/vae_encode.npz (tools/gen_vae_encode_golden.py).

The shared reference is `restate_moments` / `restate_sample` below: the encoder + quant_conv + sample over torch functional ops, in
float32 or float64, with an `emulate_bf16` switch that rounds every GEMM operand to bf16 where the bf16 engine does (the im2col'd
activations, the conv weights, q, k, V^T and the softmax rows).

Bounds.  CPU: the float32 restatement against the fixture (the reference's own float32 modules).  Where the fixture was generated the two
agree bit for bit (the same ATen kernels with the same threads: twice the largest error seen is 0), which another host's summation
order need not repeat; two float32 evaluations of the network each lie within e32 of the exact result, so the bound is 2 e32 (printed
with the error; 3.5e-6 / 4.4e-6 at the two sizes, below the 2e-5 / 5e-5 of the decoder's twin tests).  fp32 engine against the float64 restatement: 8 e32 + 1e-6 max|moments|
elementwise, e32 = the float32 restatement's own error against float64 on that case.  bf16 engine: max and rms error against float64
<= 1.5 x the error of the emulate_bf16 restatement on that case (the two differ in accumulation order and a handful of rounding sites).
dd_vae_sample: |z - z64| <= 4 * 2^-24 * 0.18215 (|mean| + std |eps|) elementwise.
"""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from duodiff_amd.autoencoder import (FrozenAutoencoderKL, synthetic_vae_encoder_state_dict, synthetic_vae_state_dict,
                                     vae_encoder_param_shapes, vae_param_shapes)

from conftest import GOLDEN, REPO, TINY

gpu = pytest.mark.gpu
SCALE = 0.18215
# sha256 over (name, fp32 bytes) of synthetic_vae_state_dict(4321), taken from the commit before the encoder existed
DECODE_WEIGHTS_SHA256 = "1ebbfadbe5ebcc081c59c012728fa56b69e0bac8e34b1122ec4728d82deb4903"


def fixture_tol(case):
    """float32 restatement vs the fixture: 2 e32 of the case (see the module docstring)"""
    _, m64, m32 = case
    return 2.0 * float(np.abs(m32.astype(np.float64) - m64).max())


# ---------------------------------------------------------------- the shared reference
def _bf16(t):
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


@torch.no_grad()
def restate_moments(x, sd, dtype=torch.float32, emulate_bf16=False):
    """encode_moments: Encoder.forward (autoencoder.py:292-317) + quant_conv (:470) -> [B,8,h,h] numpy of `dtype`"""
    p = {k: v.to(dtype) for k, v in sd.items()}
    r = _bf16 if emulate_bf16 else (lambda t: t)

    def conv(h, n, stride=1, pad=1, bias=True):
        return F.conv2d(r(h), r(p[n + ".weight"]), p[n + ".bias"] if bias else None, stride=stride, padding=pad)

    def gn(h, n, swish=True):
        h = F.group_norm(h, 32, p[n + ".weight"], p[n + ".bias"], eps=1e-6)
        return h * torch.sigmoid(h) if swish else h

    def resnet(x, n):
        h = conv(gn(x, n + ".norm1"), n + ".conv1")
        h = conv(gn(h, n + ".norm2"), n + ".conv2")
        if (n + ".nin_shortcut.weight") in p:
            x = conv(x, n + ".nin_shortcut", pad=0)
        return x + h

    def attn(x, n):
        h_ = gn(x, n + ".norm", swish=False)
        b, c, hh, ww = h_.shape
        if emulate_bf16:      # the engine's order: q, k stored as bf16; V^T without its bias, which is added behind P . V
            q, k = r(conv(h_, n + ".q", pad=0)), r(conv(h_, n + ".k", pad=0))
            v = r(conv(h_, n + ".v", pad=0, bias=False))
        else:
            q, k, v = (conv(h_, f"{n}.{t}", pad=0) for t in ("q", "k", "v"))
        w_ = torch.softmax(torch.bmm(q.reshape(b, c, -1).permute(0, 2, 1), k.reshape(b, c, -1)) * (int(c) ** (-0.5)), dim=2)
        o = torch.bmm(v.reshape(b, c, -1), r(w_).permute(0, 2, 1))
        if emulate_bf16:
            o = o + p[n + ".v.bias"][None, :, None]
        return x + conv(o.reshape(b, c, hh, ww), n + ".proj_out", pad=0)

    h = conv(torch.as_tensor(x).to(dtype), "encoder.conv_in")
    for lv in range(4):
        for j in range(2):
            h = resnet(h, f"encoder.down.{lv}.block.{j}")
        if lv != 3:
            h = conv(F.pad(h, (0, 1, 0, 1)), f"encoder.down.{lv}.downsample.conv", stride=2, pad=0)
    h = resnet(h, "encoder.mid.block_1")
    h = attn(h, "encoder.mid.attn_1")
    h = resnet(h, "encoder.mid.block_2")
    h = conv(gn(h, "encoder.norm_out"), "encoder.conv_out")
    return F.conv2d(h, p["quant_conv.weight"], p["quant_conv.bias"]).numpy()      # quant_conv runs in fp32 on the engine: no rounding


def restate_sample(moments, eps, dtype=np.float32):
    """sample (autoencoder.py:473-479) with a given eps (None: the mode)"""
    m = np.asarray(moments, dtype)
    mean, logvar = m[:, :4], np.clip(m[:, 4:], dtype(-30.0), dtype(20.0))
    if eps is None:
        return dtype(SCALE) * mean
    return dtype(SCALE) * (mean + np.exp(dtype(0.5) * logvar) * np.asarray(eps, dtype))


def uniform_image(shape, seed):
    return 2.0 * torch.rand(shape, generator=torch.Generator().manual_seed(int(seed))) - 1.0


# ---------------------------------------------------------------- fixtures, computed once
@pytest.fixture(scope="module")
def gold(golden):
    return golden("vae_encode.npz")


@pytest.fixture(scope="module")
def esd(gold):
    return synthetic_vae_encoder_state_dict(int(gold["seed"]))


@pytest.fixture(scope="module")
def full_sd(esd):
    sd = synthetic_vae_state_dict(4321)
    sd.update(esd)
    return sd


@pytest.fixture(scope="module")
def cases(gold, esd):
    """name -> (x, float64 moments, float32 moments): the references every test below shares"""
    xs = {"x64": torch.from_numpy(gold["x64"]), "x256": uniform_image((1, 3, 256, 256), gold["x256_seed"]),
          "x128": uniform_image((1, 3, 128, 128), 73), "x192": uniform_image((1, 3, 192, 192), 74)}      # x192: latent 24, HW = 576 at the attention
    out = {}
    for k, x in xs.items():
        out[k] = (x, restate_moments(x, esd, torch.float64), None if k == "x128" else restate_moments(x, esd, torch.float32))
    return out


# ---------------------------------------------------------------- CPU
def test_inventory(gold):
    shp = vae_encoder_param_shapes()
    n_values = sum(int(np.prod(s)) for s in shp.values())
    assert len(shp) == 108 and n_values == 34_163_664
    assert len(shp) == int(gold["n_tensors"]) and n_values == int(gold["n_values"])
    assert shp["encoder.conv_in.weight"] == (128, 3, 3, 3) and shp["encoder.conv_out.weight"] == (8, 512, 3, 3)
    assert shp["encoder.down.1.block.0.nin_shortcut.weight"] == (256, 128, 1, 1) and "encoder.down.3.downsample.conv.weight" not in shp
    assert shp["quant_conv.weight"] == (8, 8, 1, 1)
    assert len(vae_param_shapes()) == 140 and not set(shp) & set(vae_param_shapes())
    h = hashlib.sha256()
    for k, v in synthetic_vae_state_dict(4321).items():
        h.update(k.encode())
        h.update(v.numpy().tobytes())
    assert h.hexdigest() == DECODE_WEIGHTS_SHA256, "the decode-side synthetic weights of seed 4321 changed"


def test_restatement_matches_reference(gold, cases):
    e8 = float(np.abs(cases["x64"][2] - gold["moments8"]).max())
    e32 = float(np.abs(cases["x256"][2] - gold["moments32"]).max())
    t8, t32 = fixture_tol(cases["x64"]), fixture_tol(cases["x256"])
    print(f"float32 restatement vs fixture: max|err| 8x8 {e8:.3e} (bound 2 e32 = {t8:.3e})  32x32 {e32:.3e} (bound 2 e32 = {t32:.3e})")
    assert cases["x64"][2].shape == (2, 8, 8, 8) and cases["x256"][2].shape == (1, 8, 32, 32)
    assert e8 <= t8 and e32 <= t32, (e8, e32)
    for k, m in (("stats8", gold["moments8"]), ("stats32", gold["moments32"])):
        np.testing.assert_allclose([m.mean(dtype=np.float64), m.std(dtype=np.float64), m.min(), m.max()], gold[k], rtol=1e-6)


def _sample_bound(moments, eps):
    m = np.asarray(moments, np.float64)
    std = np.exp(0.5 * np.clip(m[:, 4:], -30.0, 20.0))
    return 4 * 2.0 ** -24 * SCALE * (np.abs(m[:, :4]) + std * np.abs(np.asarray(eps, np.float64)))


def test_sample_restatement_matches_reference(gold):
    mo, eps, z = gold["sample_moments"], gold["sample_eps"], gold["sample_z"]
    lv = mo[:, 4:]
    assert (lv < -30).any() and (lv > 20).any() and ((lv > -30) & (lv < 20)).any()
    drawn = torch.randn(eps.shape, generator=torch.Generator().manual_seed(int(gold["sample_seed"]))).numpy()
    assert np.array_equal(drawn, eps), "randn(shape, generator=manual_seed(s)) is not the reference's randn_like draw"
    got = restate_sample(mo, eps)
    assert got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - z)
    print(f"float32 sample restatement vs fixture: max|err| {err.max():.3e}")
    assert (err <= _sample_bound(mo, eps)).all()
    assert (np.abs(restate_sample(mo, eps, np.float64) - z) <= _sample_bound(mo, eps)).all()
    lo = mo.copy()
    lo[:, 4:] = -100.0
    at30 = mo.copy()
    at30[:, 4:] = -30.0
    assert np.array_equal(restate_sample(lo, eps), restate_sample(at30, eps))
    assert np.array_equal(restate_sample(mo, None), np.float32(SCALE) * mo[:, :4])


def test_state_dict_with_and_without_encoder(full_sd):
    ae = FrozenAutoencoderKL(full_sd)
    assert ae.has_encoder and len(ae._state) == 248
    part = dict(full_sd)
    part.pop("encoder.mid.attn_1.k.bias")
    ae = FrozenAutoencoderKL(part)
    assert not ae.has_encoder and len(ae._state) == 140
    for call in (lambda: ae.encode(torch.zeros(1, 3, 64, 64)), lambda: ae.encode_moments(torch.zeros(1, 3, 64, 64)),
                 lambda: ae.sample(torch.zeros(1, 8, 8, 8)), lambda: ae(torch.zeros(1, 3, 64, 64), fn="encode_moments")):
        with pytest.raises(NotImplementedError):
            call()
    bad = dict(full_sd)
    bad["encoder.conv_out.weight"] = torch.zeros(8, 512, 1, 1)
    with pytest.raises(RuntimeError, match="size mismatch"):
        FrozenAutoencoderKL(bad)


def _latent_cli(tmp_path, in_chans=4, autoencoder=True):
    import yaml
    cfg = {"model_params": dict(TINY, in_chans=in_chans)}
    if autoencoder:
        cfg["autoencoder"] = {"autoencoder_checkpoint_path": str(tmp_path / "ae.pth")}
    (tmp_path / "m.yaml").write_text(yaml.safe_dump(cfg))
    rng = np.random.default_rng(0)
    np.save(tmp_path / "img.npy", rng.uniform(-1, 1, (1, 3, 64, 64)).astype(np.float32))
    np.save(tmp_path / "img_latent.npy", rng.uniform(-1, 1, (1, 4, 8, 8)).astype(np.float32))
    np.save(tmp_path / "mask.npy", np.ones((1, 1, 64, 64), np.float32))
    np.save(tmp_path / "mask_latent.npy", np.ones((1, 1, 8, 8), np.float32))
    return ["--checkpoint_path", "/nonexistent.pth", "--batch_size", "2", "--parametrization", "predict_noise",
            "--output_folder", str(tmp_path / "out"), "--config_path", str(tmp_path / "m.yaml")]


def test_cli_rejects_invalid_encode_options_before_any_gpu_work(tmp_path):
    from duodiff_amd import dist, sampler
    f = lambda n: str(tmp_path / n)
    argv = _latent_cli(tmp_path, in_chans=3, autoencoder=False)          # a pixel-space config
    with pytest.raises(ValueError, match="latent model"):
        sampler.main(argv + ["--encode_images", "--init_image", f("img.npy"), "--strength", "0.5"])
    argv = _latent_cli(tmp_path)
    with pytest.raises(ValueError, match="--init_image or --known_image"):
        sampler.main(argv + ["--encode_images"])
    with pytest.raises(ValueError, match="does not match"):               # latents where pixels are expected
        sampler.main(argv + ["--encode_images", "--init_image", f("img_latent.npy"), "--strength", "0.5"])
    with pytest.raises(ValueError, match="does not match"):               # a latent-resolution mask
        sampler.main(argv + ["--encode_images", "--known_image", f("img.npy"), "--known_mask", f("mask_latent.npy")])
    with pytest.raises(ValueError, match="does not match"):               # pixels without the flag
        sampler.main(argv + ["--init_image", f("img.npy"), "--strength", "0.5"])
    with pytest.raises(ValueError, match="--encode_images"):
        sampler.main(argv + ["--encode_mean", "--init_image", f("img_latent.npy"), "--strength", "0.5"])
    with pytest.raises(ValueError, match="single-GPU"):
        dist.main(argv + ["--encode_images"])
    a = sampler.get_args(argv + ["--encode_images", "--known_image", f("img.npy"), "--known_mask", f("mask.npy")])
    from duodiff_amd.config import load_config
    kw = sampler.validate_region(a, load_config(tmp_path / "m.yaml"))
    assert kw["known_image"].shape == (1, 3, 64, 64) and kw["known_mask"].shape == (1, 1, 64, 64) and kw["init_image"] is None


def test_mask_reduction_is_an_8x8_minimum():
    from duodiff_amd.sampler import reduce_mask_8x8
    rng = np.random.default_rng(5)
    m = np.ones((2, 1, 32, 24), np.float32)
    holes = [(0, 0, 0), (0, 1, 2), (1, 3, 1)]                               # (image, block row, block column): one zero pixel each
    for n, by, bx in holes:
        m[n, 0, 8 * by + rng.integers(8), 8 * bx + rng.integers(8)] = 0.0
    got = reduce_mask_8x8(m)
    want = np.ones((2, 1, 4, 3), np.float32)
    for n, by, bx in holes:
        want[n, 0, by, bx] = 0.0
    assert got.dtype == np.float32 and np.array_equal(got, want)
    frac = rng.random((1, 1, 16, 16)).astype(np.float32)
    got = reduce_mask_8x8(frac)
    for by in range(2):
        for bx in range(2):
            assert got[0, 0, by, bx] == frac[0, 0, 8 * by:8 * by + 8, 8 * bx:8 * bx + 8].min()
    assert (got <= frac.reshape(1, 1, 2, 8, 2, 8).mean(axis=(3, 5))).all()      # never more known than the pixels under it


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ae_fp32(full_sd):
    return FrozenAutoencoderKL(full_sd, precision="fp32", max_chunk=2, max_latent=32).to("cuda:0")


@pytest.fixture(scope="module")
def ae_bf16(full_sd):
    return FrozenAutoencoderKL(full_sd, precision="bf16", max_chunk=2, max_latent=16).to("cuda:0")


def _bits(a, prec):
    a = np.ascontiguousarray(a, np.float32)
    return (a.view(np.uint32) >> 16).astype(np.uint16) if prec == "bf16" else a      # exact: the test data are bf16-representable


def _gather(kind, prec, B, H, W, Cn, src):
    from duodiff_amd import _lib as L
    from duodiff_amd.engine import Context
    ctx = Context.get(torch.device("cuda:0"))
    esz = 2 if prec == "bf16" else 4
    kt = 128 // esz
    kpad = (9 * (Cn if kind == 0 else 4) + kt - 1) // kt * kt
    rows, tail = B * H * W, 64
    dst = np.zeros((rows + tail) * kpad, np.uint16 if prec == "bf16" else np.float32)
    src = np.ascontiguousarray(src)
    ctx.check(ctx.lib.dd_dev_vae_gather(ctx.handle, kind, L.DD_PREC_BF16 if prec == "bf16" else L.DD_PREC_FP32, B, H, W, Cn,
                                        src.ctypes.data_as(C.c_void_p),
                                        dst.ctypes.data_as(C.c_void_p), dst.nbytes, None))
    return dst.reshape(rows + tail, kpad), kpad


def _canary(tail):
    return (tail.view(np.uint8) == 0xFF).all()


@gpu
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("H,C,B", [(2, 8, 1), (2, 128, 3), (4, 8, 3), (4, 128, 1), (6, 8, 1), (6, 128, 3)])
def test_stride2_gather_bitwise(prec, H, C, B):
    """Downsample's im2col alone: H = W = the INPUT size (H = 2: every output pixel touches the pad)"""
    rng = np.random.default_rng(H * 1000 + C + B)
    src = rng.integers(-64, 64, (B, H, H, C)).astype(np.float32) / 8.0          # exact in bf16
    Ho = H // 2
    got, kpad = _gather(0, prec, B, Ho, Ho, C, _bits(src, prec))
    want = np.zeros((B, Ho, Ho, kpad), np.float32)
    padded = np.zeros((B, H + 1, H + 1, C), np.float32)
    padded[:, :H, :H] = src
    for ky in range(3):
        for kx in range(3):
            want[..., (ky * 3 + kx) * C:(ky * 3 + kx + 1) * C] = padded[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Ho:2]
    rows = B * Ho * Ho
    assert np.array_equal(got[:rows], _bits(want.reshape(rows, kpad), prec))
    assert (got[:rows, 9 * C:] == 0).all() and _canary(got[rows:])


@gpu
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("H,B", [(1, 1), (2, 3), (5, 2)])
def test_input_gather_bitwise(prec, H, B):
    """the encoder's input path alone: NCHW 3-channel image -> 4-channel NHWC -> conv_in's im2col (K = 36 of Kpad)"""
    rng = np.random.default_rng(H * 10 + B)
    src = rng.integers(-64, 64, (B, 3, H, H)).astype(np.float32) / 64.0
    got, kpad = _gather(1, prec, B, H, H, 0, src)
    padded = np.zeros((B, H + 2, H + 2, 4), np.float32)
    padded[:, 1:H + 1, 1:H + 1, :3] = src.transpose(0, 2, 3, 1)
    want = np.zeros((B, H, H, kpad), np.float32)
    for ky in range(3):
        for kx in range(3):
            want[..., (ky * 3 + kx) * 4:(ky * 3 + kx + 1) * 4] = padded[:, ky:ky + H, kx:kx + H]
    rows = B * H * H
    assert np.array_equal(got[:rows], _bits(want.reshape(rows, kpad), prec))
    assert (got[:rows, 36:] == 0).all() and (got[:rows, 3:36:4] == 0).all() and _canary(got[rows:])


@gpu
@pytest.mark.parametrize("case", ["x64", "x256", "x192"])
def test_encode_moments_fp32(case, gold, cases, ae_fp32):
    """x192 (latent 24: GroupNorm over two whole 256-pixel chunks and a part of a third, 9 softmax elements per lane, GEMMs of M = 576) has
    no reference-generated fixture: it is held to the float64 restatement alone, under the same rule"""
    x, m64, m32 = cases[case]
    got = ae_fp32.encode_moments(x).cpu().numpy()
    fix = {"x64": gold["moments8"], "x256": gold["moments32"], "x192": m32}[case]
    tol_fix = fixture_tol(cases[case])
    assert got.shape == fix.shape and got.dtype == np.float32
    e32 = float(np.abs(m32.astype(np.float64) - m64).max())
    floor = 1e-6 * float(np.abs(m64).max())
    err = float(np.abs(got.astype(np.float64) - m64).max())
    err_fix = float(np.abs(got - fix).max())
    print(f"vae encode fp32 {case}: max|err| vs float64 {err:.3e} = {err / e32:.2f} x e32 ({e32:.3e}; bound 8 x e32 + {floor:.1e}); "
          f"vs fixture {err_fix:.3e} (bound {tol_fix + 8 * e32 + floor:.3e})")
    assert err <= 8 * e32 + floor, (err, e32)
    assert err_fix <= tol_fix + 8 * e32 + floor, err_fix


@gpu
@pytest.mark.parametrize("case", ["x64", "x128"])
def test_encode_moments_bf16(case, cases, esd, ae_bf16):
    """bf16 operands / fp32 accumulation against the restatement with the same operand roundings"""
    x, m64, _ = cases[case]
    emu = restate_moments(x, esd, torch.float32, emulate_bf16=True).astype(np.float64)
    got = ae_bf16.encode_moments(x).cpu().numpy().astype(np.float64)
    emax, erms = float(np.abs(emu - m64).max()), float(np.sqrt(np.mean((emu - m64) ** 2)))
    gmax, grms = float(np.abs(got - m64).max()), float(np.sqrt(np.mean((got - m64) ** 2)))
    print(f"vae encode bf16 {case}: engine max {gmax:.3e} rms {grms:.3e}; emulation max {emax:.3e} rms {erms:.3e}; "
          f"ratio max {gmax / emax:.2f} rms {grms / erms:.2f} (bound 1.5); moments std {m64.std():.3f}")
    assert gmax <= 1.5 * emax and grms <= 1.5 * erms, (gmax, emax, grms, erms)


@gpu
def test_sample_on_the_engine(gold, cases, ae_fp32):
    mo, eps = gold["sample_moments"], gold["sample_eps"]
    from duodiff_amd.engine import Context, _ptr, _stream_ptr
    ctx = Context.get(torch.device("cuda:0"))
    mo_d, eps_d = torch.from_numpy(mo).cuda(), torch.from_numpy(eps).cuda()
    z = torch.empty(2, 4, 4, 4, device="cuda")
    ctx.check(ctx.lib.dd_vae_sample(ctx.handle, _ptr(mo_d), _ptr(eps_d), _ptr(z), 2, 4, _stream_ptr()))
    err = np.abs(z.cpu().numpy().astype(np.float64) - restate_sample(mo, eps, np.float64))
    print(f"dd_vae_sample: max |z - z64| / bound = {(err / _sample_bound(mo, eps)).max():.3f}")
    assert (err <= _sample_bound(mo, eps)).all()
    ctx.check(ctx.lib.dd_vae_sample(ctx.handle, _ptr(mo_d), None, _ptr(z), 2, 4, _stream_ptr()))
    assert np.array_equal(z.cpu().numpy(), np.float32(SCALE) * mo[:, :4])
    # the mirror draws what the reference's randn_like draws from the same seed
    z2 = ae_fp32.sample(torch.from_numpy(mo), generator=torch.Generator().manual_seed(int(gold["sample_seed"]))).cpu().numpy()
    ctx.check(ctx.lib.dd_vae_sample(ctx.handle, _ptr(mo_d), _ptr(eps_d), _ptr(z), 2, 4, _stream_ptr()))
    assert np.array_equal(z2, z.cpu().numpy())
    # encode == sample(encode_moments) bit for bit; the mode is 0.18215 mean
    x = cases["x64"][0]
    m = ae_fp32.encode_moments(x)
    a = ae_fp32.encode(x, generator=torch.Generator().manual_seed(9))
    b = ae_fp32.sample(m, generator=torch.Generator().manual_seed(9))
    assert torch.equal(a, b) and a.shape == (2, 4, 8, 8)
    assert torch.equal(ae_fp32(x, fn="encode_moments"), m)
    assert np.array_equal(ae_fp32.encode(x, sample=False).cpu().numpy(), np.float32(SCALE) * m.cpu().numpy()[:, :4])


@gpu
def test_encode_chunking_and_batch_independence(ae_fp32):
    """B larger than the workspace chunk (max_chunk = 2): every image encodes as it does alone (bitwise)"""
    x = uniform_image((5, 3, 64, 64), 3)
    m = ae_fp32.encode_moments(x).cpu().numpy()
    for i in (0, 3, 4):
        assert np.array_equal(ae_fp32.encode_moments(x[i:i + 1]).cpu().numpy()[0], m[i]), i


@gpu
def test_encode_and_decode_share_the_workspace(cases, ae_fp32):
    x = cases["x64"][0]
    z = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(4))
    y0 = ae_fp32.decode(z).clone()
    m0 = ae_fp32.encode_moments(x).clone()
    y1 = ae_fp32.decode(z).clone()
    m1 = ae_fp32.encode_moments(x)
    assert torch.equal(y0, y1) and torch.equal(m0, m1)


@gpu
def test_encode_errors(full_sd, ae_fp32):
    from duodiff_amd.engine import Context, _ptr, _stream_ptr
    ctx, h = ae_fp32._engine()
    assert ctx.lib.dd_vae_has_encoder(h) == 1
    with pytest.raises(NotImplementedError, match="multiple of 64"):
        ae_fp32.encode_moments(torch.zeros(1, 3, 96, 96))
    with pytest.raises(ValueError, match="max_latent"):
        ae_fp32.encode_moments(torch.zeros(1, 3, 320, 320))
    with pytest.raises(RuntimeError):
        ae_fp32.encode_moments(torch.zeros(1, 4, 64, 64))
    x = torch.zeros(1, 3, 64, 64, device="cuda")
    with pytest.raises(ValueError, match="neither"):
        ctx.check(ctx.lib.dd_vae_encode(ctx.handle, h, _ptr(x), None, None, None, 1, 64, _stream_ptr()))
    assert ae_fp32.encode_moments(torch.zeros(0, 3, 64, 64)).shape == (0, 8, 8, 8)
    assert ae_fp32.encode(torch.zeros(0, 3, 64, 64)).shape == (0, 4, 8, 8)
    # a decode-only object: the mirror refuses, and so does the C ABI
    part = dict(full_sd)
    part.pop("quant_conv.bias")
    dec = FrozenAutoencoderKL(part, precision="bf16", max_chunk=1, max_latent=8).to("cuda:0")
    with pytest.raises(NotImplementedError):
        dec.encode(x)
    ctx2, h2 = dec._engine()
    assert ctx2.lib.dd_vae_has_encoder(h2) == 0
    mo = torch.empty(1, 8, 8, 8, device="cuda")
    with pytest.raises(NotImplementedError, match="decode-only"):
        ctx2.check(ctx2.lib.dd_vae_encode(ctx2.handle, h2, _ptr(x), None, _ptr(mo), None, 1, 64, _stream_ptr()))
    # an unknown encode-side name / a wrong shape is refused by the C ABI as for the decoder
    hv = C.c_void_p()
    ctx.check(ctx.lib.dd_vae_create(ctx.handle, 1, 8, C.byref(hv)))
    try:
        t = torch.zeros(128)
        one = (C.c_int64 * 1)(128)
        with pytest.raises(KeyError):
            ctx.check(ctx.lib.dd_vae_set_param(hv, b"encoder.conv_in.scale", C.c_void_p(t.data_ptr()), one, 1))
        with pytest.raises(ValueError, match="size mismatch"):
            ctx.check(ctx.lib.dd_vae_set_param(hv, b"quant_conv.bias", C.c_void_p(t.data_ptr()), one, 1))
    finally:
        ctx.lib.dd_vae_destroy(hv)


@gpu
def test_cli_encode_images_end_to_end(tmp_path, full_sd, ae_fp32):
    """--encode_images with a .png == the same run given the .npy latents ae.encode returns (and the 8x8-minimum mask), bit for bit"""
    import yaml
    from matplotlib import pyplot as plt
    from duodiff_amd import sampler
    from duodiff_amd.config import ModelParams
    from duodiff_amd.weights import synthetic_state_dict
    cfg = dict(TINY, in_chans=4)
    torch.save(dict(full_sd), tmp_path / "ae.pth")
    (tmp_path / "m.yaml").write_text(yaml.safe_dump({
        "model_params": dict(cfg, classifier_type="x"), "autoencoder": {"autoencoder_checkpoint_path": str(tmp_path / "ae.pth")}}))
    mp = ModelParams.from_dict(cfg)
    torch.save(dict(synthetic_state_dict(mp, 9)), tmp_path / "m.pth")
    rng = np.random.default_rng(11)
    plt.imsave(tmp_path / "img.png", rng.random((64, 64, 3)))
    mask = np.zeros((64, 64), np.float32)
    mask[:, :29] = 1.0                                   # the known region ends inside a latent pixel: the 8 x 8 minimum drops that column
    mask[40:, :] = 0.0
    plt.imsave(tmp_path / "mask.png", mask, cmap="gray", vmin=0, vmax=1)
    seed = 2

    def run(name, *extra):
        out = tmp_path / name
        sampler.main(["--seed", str(seed), "--checkpoint_path", str(tmp_path / "m.pth"), "--config_path", str(tmp_path / "m.yaml"),
                      "--batch_size", "2", "--parametrization", "predict_noise", "--output_folder", str(out), "--no_png",
                      "--precision", "fp32", "--use_ddim", "--ddim_steps", "6", *extra])
        return np.load(out / "samples.npy")

    px = sampler._load_image_file(tmp_path / "img.png", "--init_image", mp, True, True)
    assert px.shape == (1, 3, 64, 64) and px.min() >= -1 and px.max() <= 1
    z = ae_fp32.encode(torch.from_numpy(px), generator=torch.Generator().manual_seed(seed)).cpu().numpy()
    np.save(tmp_path / "z.npy", z)
    mpx = sampler._load_image_file(tmp_path / "mask.png", "--known_mask", mp, True, True)
    mlat = sampler.reduce_mask_8x8(mpx)
    assert set(np.unique(mpx)) == {0.0, 1.0} and mlat[0, 0, 0].tolist() == [1, 1, 1, 0, 0, 0, 0, 0] and mlat[0, 0, 5:].sum() == 0
    np.save(tmp_path / "mlat.npy", mlat)

    a = run("a", "--encode_images", "--init_image", str(tmp_path / "img.png"), "--strength", "0.5")
    b = run("b", "--init_image", str(tmp_path / "z.npy"), "--strength", "0.5")
    assert a.shape == (2, 64, 64, 3) and np.isfinite(a).all() and np.array_equal(a, b)
    c = run("c", "--encode_images", "--known_image", str(tmp_path / "img.png"), "--known_mask", str(tmp_path / "mask.png"))
    d = run("d", "--known_image", str(tmp_path / "z.npy"), "--known_mask", str(tmp_path / "mlat.npy"))
    assert np.array_equal(c, d) and not np.array_equal(a, c)
    print("cli --encode_images: init_image / strength and known_image / known_mask runs equal their .npy-latent runs bit for bit")
