"""Host-side mirror of the reference's frozen KL-VAE (models/utils/autoencoder.py:452-516).

``get_autoencoder(path)`` / ``FrozenAutoencoderKL.decode(z)`` keep the reference's call surface
(``sampler.py:141-143,320-325``); the arithmetic runs in libduodiff.so (``dd_vae_*``): z/0.18215 -> post_quant_conv ->
Decoder (ResNet / attention / upsample stack) as im2col + MFMA GEMMs.  ``encode_moments`` / ``sample`` / ``encode``
(:468-484) run the Encoder + quant_conv the same way when the state_dict carries every encode-side tensor; a checkpoint
without them gives a decode-only object whose encode methods raise NotImplementedError.
"""
import ctypes as C
from collections import OrderedDict

import torch

from . import _lib as L
from .engine import Context, PRECISIONS, _ptr, _stream_ptr

CH, CH_MULT, Z_CH = 128, (1, 2, 4, 4), 4   # ddconfig of reference get_autoencoder (autoencoder.py:503-516)


def vae_param_shapes() -> "OrderedDict[str, tuple]":
    """Decode-side tensors of the reference state_dict (post_quant_conv.* and decoder.*), name -> shape."""
    s = OrderedDict()

    def conv(n, co, ci, k):
        s[n + ".weight"] = (co, ci, k, k)
        s[n + ".bias"] = (co,)

    def norm(n, c):
        s[n + ".weight"] = (c,)
        s[n + ".bias"] = (c,)

    def res(n, ci, co):
        norm(n + ".norm1", ci); conv(n + ".conv1", co, ci, 3); norm(n + ".norm2", co); conv(n + ".conv2", co, co, 3)
        if ci != co:
            conv(n + ".nin_shortcut", co, ci, 1)

    conv("post_quant_conv", Z_CH, Z_CH, 1)
    top = CH * CH_MULT[-1]
    conv("decoder.conv_in", top, Z_CH, 3)
    res("decoder.mid.block_1", top, top)
    norm("decoder.mid.attn_1.norm", top)
    for n in ("q", "k", "v", "proj_out"):
        conv(f"decoder.mid.attn_1.{n}", top, top, 1)
    res("decoder.mid.block_2", top, top)
    cin = top
    for lv in (3, 2, 1, 0):
        cout = CH * CH_MULT[lv]
        for j in range(3):
            res(f"decoder.up.{lv}.block.{j}", cin, cout)
            cin = cout
        if lv != 0:
            conv(f"decoder.up.{lv}.upsample.conv", cin, cin, 3)
    norm("decoder.norm_out", cin)
    conv("decoder.conv_out", 3, cin, 3)
    return s


def vae_encoder_param_shapes() -> "OrderedDict[str, tuple]":
    """Encode-side tensors of the reference state_dict (encoder.* and quant_conv.*), name -> shape, in the modules' order."""
    s = OrderedDict()

    def conv(n, co, ci, k):
        s[n + ".weight"] = (co, ci, k, k)
        s[n + ".bias"] = (co,)

    def norm(n, c):
        s[n + ".weight"] = (c,)
        s[n + ".bias"] = (c,)

    def res(n, ci, co):
        norm(n + ".norm1", ci); conv(n + ".conv1", co, ci, 3); norm(n + ".norm2", co); conv(n + ".conv2", co, co, 3)
        if ci != co:
            conv(n + ".nin_shortcut", co, ci, 1)

    conv("encoder.conv_in", CH, 3, 3)
    cin = CH
    for lv in range(4):
        cout = CH * CH_MULT[lv]
        for j in range(2):
            res(f"encoder.down.{lv}.block.{j}", cin, cout)
            cin = cout
        if lv != 3:
            conv(f"encoder.down.{lv}.downsample.conv", cin, cin, 3)
    res("encoder.mid.block_1", cin, cin)
    norm("encoder.mid.attn_1.norm", cin)
    for n in ("q", "k", "v", "proj_out"):
        conv(f"encoder.mid.attn_1.{n}", cin, cin, 1)
    res("encoder.mid.block_2", cin, cin)
    norm("encoder.norm_out", cin)
    conv("encoder.conv_out", 2 * Z_CH, cin, 3)
    conv("quant_conv", 2 * Z_CH, 2 * Z_CH, 1)
    return s


def _synthetic(shapes, seed):
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    sd = OrderedDict()
    for name, shp in shapes.items():
        if name.endswith(".bias"):
            t = 0.02 * torch.randn(shp, generator=g)
        elif len(shp) == 1:
            t = 1.0 + 0.1 * torch.randn(shp, generator=g)
        else:
            fan_in = shp[1] * shp[2] * shp[3]
            t = torch.randn(shp, generator=g) / (fan_in ** 0.5)
        sd[name] = t.to(torch.float32).contiguous()
    return sd


def synthetic_vae_encoder_state_dict(seed: int = 8765) -> "OrderedDict[str, torch.Tensor]":
    """Seeded fp32 encode-side weights, drawn as synthetic_vae_state_dict draws the decode side but from a generator of their own
    (the decode-side weights of a seed do not depend on whether the encoder's are asked for)."""
    return _synthetic(vae_encoder_param_shapes(), seed)


def synthetic_vae_state_dict(seed: int = 4321) -> "OrderedDict[str, torch.Tensor]":
    """Seeded fp32 decode-side weights (no checkpoint exists offline): conv W ~ N(0, 1/fan_in), b ~ N(0, 0.02^2),
    GroupNorm gamma ~ 1 + N(0, 0.1^2), beta ~ N(0, 0.02^2)."""
    return _synthetic(vae_param_shapes(), seed)


class FrozenAutoencoderKL:
    """``scale_factor`` is fixed to the reference's 0.18215 in the engine.  ``has_encoder``: the state_dict carried every encode-side
    tensor (vae_encoder_param_shapes); otherwise the object decodes only."""

    def __init__(self, state_dict=None, scale_factor=0.18215, precision="bf16", max_chunk=4, max_latent=32):
        if abs(scale_factor - 0.18215) > 1e-12:
            raise NotImplementedError("the engine's decode uses the reference scale_factor 0.18215")
        self.scale_factor, self.precision = scale_factor, precision
        self.max_chunk, self.max_latent = int(max_chunk), int(max_latent)
        self.embed_dim = 4
        self._state, self._handle, self._ctx, self._device = None, None, None, None
        self.has_encoder = False
        if state_dict is not None:
            self.load_state_dict(state_dict)

    def load_state_dict(self, state_dict, strict=True):
        want = vae_param_shapes()
        missing = [k for k in want if k not in state_dict]
        if strict and missing:
            raise RuntimeError(f"Error(s) in loading state_dict for FrozenAutoencoderKL: missing keys {missing}")
        enc = vae_encoder_param_shapes()
        self.has_encoder = all(k in state_dict for k in enc)      # all of them or none: a partial set loads decode-only
        if self.has_encoder:
            want.update(enc)
        sd = OrderedDict()
        for k, shp in want.items():
            t = torch.as_tensor(state_dict[k]).detach().to("cpu", torch.float32)
            if tuple(t.shape) != tuple(shp):
                raise RuntimeError(f"size mismatch for {k}: {tuple(t.shape)} vs {tuple(shp)}")
            sd[k] = t.contiguous()
        self._state, self._handle = sd, None
        return [], []

    def eval(self):
        return self

    def requires_grad_(self, flag=False):
        return self

    def to(self, device):
        self._device = torch.device(device)
        return self

    @property
    def device(self):
        return self._device or torch.device("cuda", torch.cuda.current_device())

    def _engine(self):
        if self._state is None:
            raise RuntimeError("FrozenAutoencoderKL has no weights: call load_state_dict first")
        if self._handle is None:
            ctx = Context.get(self.device)
            h = C.c_void_p()
            ctx.check(ctx.lib.dd_vae_create(ctx.handle, self.max_chunk, self.max_latent, C.byref(h)))
            for k, t in self._state.items():
                shape = (C.c_int64 * t.dim())(*t.shape)
                ctx.check(ctx.lib.dd_vae_set_param(h, k.encode(), C.c_void_p(t.data_ptr()), shape, t.dim()))
            with torch.cuda.device(ctx.device):
                ctx.check(ctx.lib.dd_vae_finalize(h, PRECISIONS[self.precision]))
            self._handle, self._ctx = h, ctx
        return self._ctx, self._handle

    def decode(self, z, stream=None):
        """reference autoencoder.py:486-490: [B,4,h,h] latents -> [B,3,8h,8h] images (fp32, on the device)."""
        ctx, h = self._engine()
        z = z.to(self.device, torch.float32).contiguous()
        B, c, hh, ww = z.shape
        if c != 4 or hh != ww:
            raise RuntimeError(f"expected latents [B,4,h,h], got {tuple(z.shape)}")
        out = torch.empty(B, 3, 8 * hh, 8 * ww, device=z.device, dtype=torch.float32)
        if B == 0:
            return out
        ctx.check(ctx.lib.dd_vae_decode(ctx.handle, h, _ptr(z), _ptr(out), B, hh, _stream_ptr(stream)))
        return out

    def _need_encoder(self):
        if not self.has_encoder:
            raise NotImplementedError("this autoencoder was loaded without the encoder tensors (encoder.*, quant_conv.*): decode only")

    def _eps(self, shape, generator):
        """the reference's torch.randn_like(mean) (autoencoder.py:477), drawn on the CPU and copied over"""
        return torch.randn(shape, generator=generator).to(self.device, torch.float32).contiguous()

    def _encode(self, x, eps, want_moments, want_z, stream):
        self._need_encoder()
        ctx, h = self._engine()
        x = x.to(self.device, torch.float32).contiguous()
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3]:
            raise RuntimeError(f"expected images [B,3,H,H], got {tuple(x.shape)}")
        B, hw = x.shape[0], x.shape[2]
        moments = torch.empty(B, 2 * Z_CH, hw // 8, hw // 8, device=x.device, dtype=torch.float32) if want_moments else None
        z = torch.empty(B, Z_CH, hw // 8, hw // 8, device=x.device, dtype=torch.float32) if want_z else None
        if B > 0:
            e = eps(z.shape) if (want_z and eps is not None) else None
            ctx.check(ctx.lib.dd_vae_encode(ctx.handle, h, _ptr(x), _ptr(e), _ptr(moments), _ptr(z), B, hw, _stream_ptr(stream)))
        return moments, z

    def encode_moments(self, x, stream=None):
        """reference autoencoder.py:468-471: [B,3,8h,8h] images in [-1, 1] -> [B,8,h,h] (mean | logvar), fp32 on the device."""
        return self._encode(x, None, True, False, stream)[0]

    def sample(self, moments, generator=None, stream=None):
        """reference autoencoder.py:473-479: z = 0.18215 (mean + exp(0.5 clamp(logvar, -30, 20)) eps), eps = randn_like(mean)
        from `generator` (None: the global CPU generator, as the reference draws)."""
        self._need_encoder()
        ctx, _ = self._engine()
        moments = moments.to(self.device, torch.float32).contiguous()
        if moments.dim() != 4 or moments.shape[1] != 2 * Z_CH or moments.shape[2] != moments.shape[3]:
            raise RuntimeError(f"expected moments [B,8,h,h], got {tuple(moments.shape)}")
        B, hh = moments.shape[0], moments.shape[2]
        z = torch.empty(B, Z_CH, hh, hh, device=moments.device, dtype=torch.float32)
        if B > 0 and hh > 0:
            e = self._eps(z.shape, generator)
            ctx.check(ctx.lib.dd_vae_sample(ctx.handle, _ptr(moments), _ptr(e), _ptr(z), B, hh, _stream_ptr(stream)))
        return z

    def encode(self, x, generator=None, sample=True, stream=None):
        """reference autoencoder.py:481-484: sample(encode_moments(x)) in one engine call; sample=False: the mode, 0.18215 mean."""
        return self._encode(x, (lambda shp: self._eps(shp, generator)) if sample else None, False, True, stream)[1]

    def __call__(self, inputs, fn="decode"):
        if fn == "decode":
            return self.decode(inputs)
        if fn == "encode":
            return self.encode(inputs)
        if fn == "encode_moments":
            return self.encode_moments(inputs)
        raise NotImplementedError(fn)

    def __del__(self):
        try:
            if self._handle is not None and self._handle.value:
                self._ctx.lib.dd_vae_destroy(self._handle)
                self._handle = None
        except Exception:
            pass


def get_autoencoder(pretrained_path, scale_factor=0.18215, precision="bf16"):
    """reference autoencoder.py:503-516: build the fixed-config KL-VAE and load its checkpoint (the encoder too when the
    checkpoint carries every one of its tensors)."""
    sd = torch.load(pretrained_path, map_location="cpu")
    return FrozenAutoencoderKL(sd, scale_factor, precision=precision)
