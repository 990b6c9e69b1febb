"""Thin object layer over the C ABI: one Context per (process, GPU), Models built from a
reference-style state_dict.  torch tensors are containers for device memory and streams only.
"""
import contextlib
import ctypes as C
from typing import NamedTuple

import numpy as np
import torch

from . import _lib as L
from .config import ModelParams

_ERR_CLASS = {
    L.DD_ERR_INVALID: ValueError,
    L.DD_ERR_NOT_FOUND: KeyError,
    L.DD_ERR_STATE: RuntimeError,
    L.DD_ERR_HIP: RuntimeError,
    L.DD_ERR_NOMEM: MemoryError,
    L.DD_ERR_UNSUPPORTED: NotImplementedError,
}

PRECISIONS = {"bf16": L.DD_PREC_BF16, "fp32": L.DD_PREC_FP32}


def _stream_ptr(stream=None):
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class Context:
    """dd_ctx: bound to one device.  Creation fails loudly without a gfx950 GPU."""

    _per_device = {}

    def __init__(self, device=None):
        self.lib = L.load()
        if not torch.cuda.is_available():
            raise L.EngineUnavailable("no GPU visible: the DuoDiff engine runs only on MI355X (gfx950)")
        self.device = torch.cuda.current_device() if device is None else torch.device(device).index or 0
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            rc = self.lib.dd_ctx_create(int(self.device), C.byref(h))
        if rc != L.DD_OK:
            raise L.EngineUnavailable(f"dd_ctx_create(device={self.device}) failed with status {rc} "
                                      "(needs a gfx950 device and a working HIP runtime)")
        self.handle = h

    @classmethod
    def get(cls, device=None):
        idx = torch.cuda.current_device() if device is None else (torch.device(device).index or 0)
        if idx not in cls._per_device:
            cls._per_device[idx] = cls(idx)
        return cls._per_device[idx]

    def check(self, rc):
        if rc == L.DD_OK:
            return
        msg = self.lib.dd_last_error(self.handle)
        msg = msg.decode() if msg else f"status {rc}"
        raise _ERR_CLASS.get(rc, RuntimeError)(msg)

    def side_stream(self, device):
        if getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream(device=device)
        return self._side

    def sync(self, stream=None):
        self.check(self.lib.dd_sync(self.handle, _stream_ptr(stream)))

    def ddpm_step(self, x, eps, z, t, variance="beta_tilde", out=None, stream=None):
        """x' = postprocessing(eps, x, t) (reference sampler.py:47-56) on device tensors."""
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
        out = torch.empty_like(x) if out is None else out
        var = L.DD_VAR_BETA if variance == "beta" else L.DD_VAR_BETA_TILDE
        self.check(self.lib.dd_ddpm_step(self.handle, _ptr(x), _ptr(eps.contiguous()),
                                         _ptr(z.contiguous() if z is not None else None), int(t), var,
                                         _ptr(out), x.numel(), _stream_ptr(stream)))
        return out

    def ddpm_step_coef(self, x, eps, z, c1, c2, sigma, out=None, stream=None):
        """x' = c1 * (x - c2 * eps) + sigma * z with caller-supplied scalars (any schedule; ddpm_core.py:190-193)."""
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
        out = torch.empty_like(x) if out is None else out
        self.check(self.lib.dd_ddpm_step_coef(self.handle, _ptr(x), _ptr(eps.contiguous()),
                                              _ptr(z.contiguous() if z is not None else None), float(c1), float(c2),
                                              float(sigma), _ptr(out), x.numel(), _stream_ptr(stream)))
        return out

    def to_images(self, x, out=None, stream=None):
        """(x + 1) / 2 as [B,H,W,C] (reference sampler.py:145-146), on the device."""
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4 and x.shape[2] == x.shape[3]
        B, Cc, S, _ = x.shape
        out = torch.empty(B, S, S, Cc, device=x.device, dtype=torch.float32) if out is None else out
        self.check(self.lib.dd_to_images(self.handle, _ptr(x), _ptr(out), B, Cc, S, _stream_ptr(stream)))
        return out

    def early_exit_select(self, outputs, eps, classifier_outputs, threshold, stream=None):
        """eesampler.py:61-71 on device tensors -> (model_output [B,...], indices int32 [B], batch-mean errors [depth])."""
        depth, B = classifier_outputs.shape
        mo = torch.empty_like(eps)
        idx = torch.empty(B, device=eps.device, dtype=torch.int32)
        err = torch.empty(depth, device=eps.device, dtype=torch.float32)
        self.check(self.lib.dd_early_exit_select(self.handle, _ptr(outputs), _ptr(eps), _ptr(classifier_outputs),
                                                 float(threshold), depth, B, eps.numel() // max(B, 1), _ptr(mo), _ptr(idx),
                                                 _ptr(err), _stream_ptr(stream)))
        return mo, idx, err

    def affine_step(self, x, m, z, a, b, c, out=None, stream=None):
        """out = a*x + b*m + c*z on device tensors (z may be None)."""
        out = torch.empty_like(x) if out is None else out
        self.check(self.lib.dd_affine_step(self.handle, _ptr(x.contiguous()), _ptr(m.contiguous()),
                                           _ptr(z.contiguous() if z is not None else None), float(a), float(b),
                                           float(c), _ptr(out), x.numel(), _stream_ptr(stream)))
        return out

    def multistep_step(self, x, m, z, h, a, b, c, d, p, q, use_hist, out=None, stream=None):
        """out = a*x + b*m [+ d*h if use_hist] [+ c*z if z is not None], then h <- p*x + q*m (dd_multistep_step): one DPM-Solver++ row,
        h updated in place."""
        out = torch.empty_like(x) if out is None else out
        assert h.is_cuda and h.dtype == torch.float32 and h.is_contiguous() and h.numel() == x.numel()
        self.check(self.lib.dd_multistep_step(self.handle, _ptr(x.contiguous()), _ptr(m.contiguous()),
                                              _ptr(z.contiguous() if z is not None else None), _ptr(h), float(a), float(b), float(c),
                                              float(d), float(p), float(q), int(bool(use_hist)), _ptr(out), x.numel(), _stream_ptr(stream)))
        return out

    def threshold_step(self, x, m, z, h, threshold, a, b, c, d, p, q, use_hist, out=None, stream=None):
        """The thresholded multistep row on device tensors [B,C,S,S] (dd_threshold_step): x0 = p*x + q*m, xh = x0 clipped (threshold:
        an X0Threshold), out = a*x + b*xh [+ d*h if use_hist] [+ c*z if z is not None], then h <- xh.  a, b: the UNFOLDED row.  out may be x."""
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4 and x.shape[2] == x.shape[3]
        B, Cc, S, _ = x.shape
        for v in (m, h) + ((z,) if z is not None else ()):
            assert v.is_cuda and v.dtype == torch.float32 and v.is_contiguous() and v.shape == x.shape
        out = torch.empty_like(x) if out is None else out
        thr = threshold_struct(threshold)
        self.check(self.lib.dd_threshold_step(self.handle, _ptr(x), _ptr(m), _ptr(z), _ptr(h), C.byref(thr), float(a), float(b), float(c),
                                              float(d), float(p), float(q), int(bool(use_hist)), _ptr(out), B, Cc, S, _stream_ptr(stream)))
        return out

    def known_blend(self, x, x0, mask, z2, ka, kb, out=None, stream=None):
        """The known-region rule on device tensors (dd_known_blend): kn = ka*x0 [+ kb*z2 if kb != 0 and z2 is not None];
        out = x where mask == 0, else mask*kn + (1 - mask)*x.  x, x0 [B,C,S,S], mask [B,1,S,S]; out may be x."""
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4 and x.shape[2] == x.shape[3]
        B, Cc, S, _ = x.shape
        for v, shape in ((x0, (B, Cc, S, S)), (mask, (B, 1, S, S))) + (((z2, (B, Cc, S, S)),) if z2 is not None else ()):
            assert v.is_cuda and v.dtype == torch.float32 and v.is_contiguous() and tuple(v.shape) == shape
        out = torch.empty_like(x) if out is None else out
        self.check(self.lib.dd_known_blend(self.handle, _ptr(x), _ptr(x0), _ptr(mask), _ptr(z2), float(ka), float(kb), _ptr(out),
                                           B, Cc, S, _stream_ptr(stream)))
        return out

    def jump_step(self, x, z, ja, jc, out=None, stream=None):
        """The resampling jump on device tensors (dd_jump_step): out = ja*x [+ jc*z if z is not None], each product rounded on its own.
        out may be x."""
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
        if z is not None:
            assert z.is_cuda and z.dtype == torch.float32 and z.is_contiguous() and z.numel() == x.numel()
        out = torch.empty_like(x) if out is None else out
        self.check(self.lib.dd_jump_step(self.handle, _ptr(x), _ptr(z), float(ja), float(jc), _ptr(out), x.numel(), _stream_ptr(stream)))
        return out

    def _seeds_tensor(self, seeds, device=None):
        """a sequence of ints in [0, 2^64) -> the uint64 seeds on the device (an int64 tensor of the same bits)"""
        seeds = [int(s) for s in seeds]
        if any(not 0 <= s < 1 << 64 for s in seeds):
            raise ValueError("image seeds must lie in [0, 2^64)")
        host = torch.from_numpy(np.array(seeds, np.uint64).view(np.int64))
        return host.to(torch.device("cuda", self.device) if device is None else device)

    def set_image_seeds(self, seeds):
        """dd_set_image_seeds: while set, image i of every call that draws device noise (the sample_*_loop functions, Model.sample_step
        with noise="philox") draws under seeds[i] (a sequence of ints, one per image of the call) with image-local pixel ids -- exactly
        what the plain call with B = 1 and seed = seeds[i] draws; the call's own seed is unused.  None clears.  For one call or a few:
        `with ctx.image_seeds(seeds): ...`."""
        if seeds is None:
            self.check(self.lib.dd_set_image_seeds(self.handle, None, 0))
            self._image_seeds = None
            return
        t = self._seeds_tensor(seeds)
        if t.numel() == 0:
            raise ValueError("image seeds: an empty sequence (None clears)")
        self.check(self.lib.dd_set_image_seeds(self.handle, _ptr(t), t.numel()))
        self._image_seeds = t               # (the engine reads the array at every call while it is set)

    @contextlib.contextmanager
    def image_seeds(self, seeds, stream=None):
        """Per-image seeds for the calls inside the block: set before it, cleared behind it whatever happens (seeds None: a plain block).
        stream: the stream those calls are given, where it is not the current one."""
        if seeds is None:
            yield
            return
        self.set_image_seeds(seeds)
        try:
            yield
        finally:
            t = self._image_seeds
            dev = torch.device("cuda", self.device)
            for s in (stream, torch.cuda.current_stream(dev), getattr(self, "_side", None)):     # the streams a call may have read them on
                if s is not None:
                    t.record_stream(s)
            self.set_image_seeds(None)

    def noise_images(self, B, C, S, seed=0, image_seeds=None, counter=0, out=None, stream=None):
        """dd_noise_images: x_T [B, C, S, S] drawn on the device under `seed` with batch-wide pixel ids, or (image_seeds: B ints) image i
        under image_seeds[i] with image-local ids -- then image i is what the B = 1 call with seed = image_seeds[i] returns.  The draw has a
        stream word of its own: independent of every step's noise under the same seeds."""
        dev = torch.device("cuda", self.device)
        out = torch.empty(int(B), int(C), int(S), int(S), device=dev, dtype=torch.float32) if out is None else out
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (B, C, S, S)
        sd = None
        if image_seeds is not None:
            sd = self._seeds_tensor(image_seeds, out.device)
            if sd.numel() != B:
                raise ValueError(f"{sd.numel()} image seeds for {B} images")
        self.check(self.lib.dd_noise_images(self.handle, int(seed) & (2 ** 64 - 1), _ptr(sd), int(counter), _ptr(out), int(B), int(C), int(S),
                                            _stream_ptr(stream)))
        if sd is not None:
            sd.record_stream(stream if stream is not None else torch.cuda.current_stream(out.device))
        return out

    def set_num_cus(self, n):
        """CU count this context's persistent GEMM grids are sized for (CU-masked streams)."""
        self.check(self.lib.dd_set_num_cus(self.handle, int(n)))

    def last_sample_timing(self):
        buf = (C.c_float * 3)()
        self.check(self.lib.dd_last_sample_timing(self.handle, buf))
        return tuple(buf)

    def __del__(self):
        try:
            if getattr(self, "handle", None) and self.handle.value:
                self.lib.dd_ctx_destroy(self.handle)
                self.handle = C.c_void_p(0)
        except Exception:
            pass


def schedule_tables():
    """The engine's own schedule tables (host arithmetic, usable without a GPU)."""
    lib = L.load()
    names = ["betas", "alphas", "alphas_bar", "alphas_bar_previous", "betas_tilde",
             "betas_tilde_scheduler", "c1", "c2", "sigma"]
    out = {}
    for i, n in enumerate(names):
        a = np.empty(1000, np.float32)
        rc = lib.dd_schedule_table(i, a.ctypes.data_as(C.POINTER(C.c_float)))
        if rc != L.DD_OK:
            raise RuntimeError(f"dd_schedule_table({i}) -> {rc}")
        out[n] = a
    return out


def build_schedule(beta_init=1e-4, beta_final=0.02, beta_steps=1000):
    """NoiseScheduler.__init__ tables (ddpm_core.py:56-70) for any schedule, from the engine's host arithmetic."""
    lib = L.load()
    n = int(beta_steps)
    names = ["betas", "alphas", "alphas_bar", "alpha_bar_prev", "betas_tilde"]
    arrs = [np.empty(n, np.float32) for _ in names]
    rc = lib.dd_schedule_build(float(beta_init), float(beta_final), n, *[a.ctypes.data_as(C.POINTER(C.c_float)) for a in arrs])
    if rc != L.DD_OK:
        raise ValueError(f"dd_schedule_build({beta_init}, {beta_final}, {beta_steps}) -> {rc}")
    return dict(zip(names, arrs))


class Model:
    """dd_model: U-ViT weights packed on the device + its activation workspace."""

    def __init__(self, ctx: Context, mp: ModelParams, max_batch: int):
        self.ctx, self.mp, self.max_batch = ctx, mp, int(max_batch)
        cfg = L.dd_config(mp.img_size, mp.patch_size, mp.in_chans, mp.embed_dim, mp.depth, mp.num_heads,
                          mp.mlp_ratio, mp.num_classes, int(mp.normalize_timesteps), self.max_batch,
                          int(mp.qkv_bias), int(mp.mlp_time_embed))
        h = C.c_void_p()
        ctx.check(ctx.lib.dd_model_create(ctx.handle, C.byref(cfg), C.byref(h)))
        self.handle = h
        self.finalized = False
        self.precision = None

    def enable_early_exit(self, classifier_type="mlp_probe_per_layer"):
        kinds = {"mlp_probe_per_layer": L.DD_EE_MLP_PER_LAYER, "mlp_probe_per_timestep": L.DD_EE_MLP_PER_TIMESTEP,
                 "mlp_probe_per_layer_per_timestep": L.DD_EE_MLP_PER_LAYER_PER_TIMESTEP,
                 "attention_probe": L.DD_EE_ATTENTION_PROBE}
        if classifier_type not in kinds:
            raise ValueError(f"Unknown classifier type: {classifier_type}")
        self.ctx.check(self.ctx.lib.dd_model_enable_early_exit(self.handle, kinds[classifier_type]))

    def forward_early_exit(self, x, t, y=None, t_vec=None, stream=None):
        """(eps [B,C,S,S], classifier_outputs [depth,B], outputs [depth,B,C,S,S]) of EarlyExitUViT.forward."""
        B, depth = x.shape[0], self.mp.depth
        eps = torch.empty_like(x)
        cls = torch.empty(depth, B, device=x.device, dtype=torch.float32)
        outs = torch.empty((depth,) + tuple(x.shape), device=x.device, dtype=torch.float32)
        self.ctx.check(self.ctx.lib.dd_forward_early_exit(self.ctx.handle, self.handle, _ptr(x), float(t), _ptr(t_vec), _ptr(y),
                                                          _ptr(eps), _ptr(cls), _ptr(outs), B, _stream_ptr(stream)))
        return eps, cls, outs

    def set_param(self, name, tensor):
        t = tensor.detach().to("cpu", torch.float32).contiguous()
        shape = (C.c_int64 * t.dim())(*t.shape)
        self.ctx.check(self.ctx.lib.dd_model_set_param(self.handle, name.encode(), C.c_void_p(t.data_ptr()),
                                                       shape, t.dim()))

    def finalize(self, precision="bf16"):
        with torch.cuda.device(self.ctx.device):
            self.ctx.check(self.ctx.lib.dd_model_finalize(self.handle, PRECISIONS[precision]))
        self.finalized, self.precision = True, precision

    def forward(self, x, t, y=None, out=None, t_vec=None, stream=None):
        """eps = model(x, t, y).  t: the common timestep; t_vec: optional [B] fp32 device tensor."""
        B = x.shape[0]
        out = torch.empty_like(x) if out is None else out
        self.ctx.check(self.ctx.lib.dd_forward(self.ctx.handle, self.handle, _ptr(x), float(t), _ptr(t_vec),
                                               _ptr(y), _ptr(out), B, _stream_ptr(stream)))
        return out

    def forward_guided(self, x, t, y, scale, null_label, out=None, stream=None):
        """Classifier-free guided eps = eps_c + scale * (eps_c - eps_u) at timestep t (dd_forward_guided): the backbone runs 2 B rows,
        x with labels y, then x with null_label; max_batch must hold them."""
        B = x.shape[0]
        out = torch.empty_like(x) if out is None else out
        g = guidance_struct((scale, null_label))
        self.ctx.check(self.ctx.lib.dd_forward_guided(self.ctx.handle, self.handle, _ptr(x), float(t), _ptr(y), C.byref(g),
                                                      _ptr(out), B, _stream_ptr(stream)))
        return out

    def forward_cached(self, x, t, y=None, *, blocks, op, w=0.0, guidance=None, out=None, stream=None):
        """eps = model(x, t, y) with block caching (dd_forward_cached), on the whole-batch chain's cache of this model.  blocks = K: the
        deep blocks K .. depth - 1 - K.  op 0: a refresh -- the full forward, which stores the deep blocks' output (the stored one before it
        becomes prev); op 1: a reuse -- the deep blocks do not run, the out-block behind them takes the stored output; op 2: a reuse on
        last + w (last - prev).  guidance = (scale, null_label): classifier-free guidance, the cache then holds the 2 B rows."""
        B = x.shape[0]
        out = torch.empty_like(x) if out is None else out
        g = C.byref(guidance_struct(guidance)) if guidance is not None else None
        self.ctx.check(self.ctx.lib.dd_forward_cached(self.ctx.handle, self.handle, _ptr(x), float(t), _ptr(y), g, int(blocks), int(op),
                                                      float(w), _ptr(out), B, _stream_ptr(stream)))
        return out

    def forward_autoguided(self, x, t, y, guide, scale, out=None, stream=None):
        """Autoguided eps = eps_main + scale * (eps_main - eps_guide) at timestep t (dd_forward_autoguided): `guide` (a Model of the same
        image geometry) and this model run the same B rows; y is required iff either model is class-conditional, and each model takes it
        iff it is.  guide is this model itself: the plain forward."""
        B = x.shape[0]
        out = torch.empty_like(x) if out is None else out
        g = L.dd_autoguidance(guide.handle, float(scale))
        self.ctx.check(self.ctx.lib.dd_forward_autoguided(self.ctx.handle, self.handle, _ptr(x), float(t), _ptr(y), C.byref(g),
                                                          _ptr(out), B, _stream_ptr(stream)))
        return out

    def forward_perturbed(self, x, t, y, scale, layers, out=None, stream=None):
        """Perturbed-attention guided eps = eps + scale * (eps - eps_perturbed) at timestep t (dd_forward_perturbed): the backbone runs
        2 B rows, x as it is, then x with identity attention in the blocks of `layers` (block indices in forward order, or their bit
        mask); max_batch must hold them.  y as in forward: labels of a class-conditional model, else None."""
        B = x.shape[0]
        out = torch.empty_like(x) if out is None else out
        p = L.dd_pag(float(scale), layer_mask(layers), 0)
        self.ctx.check(self.ctx.lib.dd_forward_perturbed(self.ctx.handle, self.handle, _ptr(x), float(t), _ptr(y), C.byref(p),
                                                         _ptr(out), B, _stream_ptr(stream)))
        return out

    def sample_step(self, x, t, y=None, z=None, noise="buffer", seed=0, variance="beta_tilde", eps_out=None,
                    stream=None):
        mode = {"none": L.DD_NOISE_NONE, "buffer": L.DD_NOISE_BUFFER, "philox": L.DD_NOISE_PHILOX}[noise]
        if mode == L.DD_NOISE_BUFFER and z is None:
            mode = L.DD_NOISE_NONE
        var = L.DD_VAR_BETA if variance == "beta" else L.DD_VAR_BETA_TILDE
        self.ctx.check(self.ctx.lib.dd_sample_step(self.ctx.handle, self.handle, _ptr(x), int(t), _ptr(y), mode,
                                                   _ptr(z), int(seed), var, _ptr(eps_out), x.shape[0],
                                                   _stream_ptr(stream)))
        return x

    PROFILE_KINDS = {"dominant": L.DD_PROF_DOMINANT, "block_tail": L.DD_PROF_BLOCK_TAIL, "fc1": L.DD_PROF_FC1, "rowlin": L.DD_PROF_ROWLIN,
                     "qkv_attention": L.DD_PROF_QKV_ATTENTION, "splitk": L.DD_PROF_SPLITK}

    def profile_steps(self, x, t_start=699, steps=10, y=None, stream=None, kind="dominant"):
        """Average ms per launch of one kernel family measured in context (event pairs around every such launch of `steps` eager steps);
        kind: "dominant" (the fused block tail where the model has one, else the fc1 GEMM) or one of PROFILE_KINDS."""
        ms, n = C.c_float(), C.c_int()
        self.ctx.check(self.ctx.lib.dd_profile_select(self.ctx.handle, self.PROFILE_KINDS[kind]))
        self.ctx.check(self.ctx.lib.dd_profile_steps(self.ctx.handle, self.handle, _ptr(x), _ptr(y), int(t_start), int(steps),
                                                     x.shape[0], _stream_ptr(stream), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def profile_steps_chained(self, x, t_start=699, steps=10, y=None, stream=None, kind="dominant"):
        """The same with the batch split into dd_sample's two half-batch chains (the caller's stream + the context's side stream):
        average ms of a half-batch launch of the dominant kernel while the other chain runs beside it."""
        ms, n = C.c_float(), C.c_int()
        self.ctx.check(self.ctx.lib.dd_profile_select(self.ctx.handle, self.PROFILE_KINDS[kind]))
        self.ctx.check(self.ctx.lib.dd_profile_steps_chained(self.ctx.handle, self.handle, _ptr(x), _ptr(y), int(t_start), int(steps),
                                                             x.shape[0], _stream_ptr(stream), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def bench_gemm(self, B, iters=20, stream=None):
        ms, fl = C.c_float(), C.c_double()
        self.ctx.check(self.ctx.lib.dd_bench_gemm(self.ctx.handle, self.handle, int(B), int(iters),
                                                  _stream_ptr(stream), C.byref(ms), C.byref(fl)))
        return ms.value, fl.value

    def __del__(self):
        try:
            if getattr(self, "handle", None) and self.handle.value:
                self.ctx.lib.dd_model_destroy(self.handle)
                self.handle = C.c_void_p(0)
        except Exception:
            pass


def guidance_struct(guidance):
    """(scale, null_label) -> the C ABI's dd_guidance"""
    scale, null_label = guidance
    return L.dd_guidance(float(scale), int(null_label))


class Autoguidance(NamedTuple):
    """A loop's `guidance` argument for autoguidance: every step of a model other than `guide` (a Model of the same image geometry) also
    runs `guide` on the same rows and uses eps_main + scale * (eps_main - eps_guide); a step `guide` itself runs is the unguided step."""
    guide: "Model"
    scale: float


def layer_mask(layers):
    """Block indices in forward order (in_blocks, mid_block, out_blocks), or their bit mask as an int -> the bit mask"""
    if isinstance(layers, (int, np.integer)):
        mask = int(layers)
    else:
        mask = 0
        for i in layers:
            if not 0 <= int(i) < 32:
                raise ValueError(f"block index {i} outside [0, 32)")
            mask |= 1 << int(i)
    if not 0 <= mask < 1 << 32:
        raise ValueError("block mask outside 32 bits")
    return mask


class Perturbed(NamedTuple):
    """A loop's `guidance` argument for perturbed-attention guidance: every step runs its 2 B rows [x | x], the second half with identity
    attention in the masked blocks of the running model (layers_first for the loop's first model, layers_late for its late model: block
    indices or bit masks), and uses eps + scale * (eps - eps_perturbed).  Not with a known region or x0 thresholding."""
    scale: float
    layers_first: object
    layers_late: object = 0


class KnownRegion(NamedTuple):
    """A loop's `region` argument: after every step, x' is finished as mask * (ka[k] x0 + kb[k] z2) + (1 - mask) x' (x' kept bit for bit
    where mask == 0).  x0 [B,C,S,S] and mask [B,1,S,S] are fp32 device tensors, ka / kb one value per step of the call
    (sampler.known_rows)."""
    x0: torch.Tensor
    mask: torch.Tensor
    ka: np.ndarray
    kb: np.ndarray


class X0Threshold(NamedTuple):
    """A thresholded loop's `threshold` argument.  mode "static": x0 is clamped to [-range, range]; mode "dynamic": each image's x0 is
    clamped to +-s and divided by s, s = the `quantile` of its |x0| (linear interpolation), at least 1 and at most s_max."""
    mode: str
    quantile: float = 0.995
    range: float = 1.0
    s_max: float = float("inf")


def threshold_struct(threshold):
    """X0Threshold -> the C ABI's dd_x0_threshold (the engine checks the values)"""
    if threshold.mode not in ("static", "dynamic"):
        raise ValueError(f"threshold mode must be 'static' or 'dynamic', not {threshold.mode!r}")
    return L.dd_x0_threshold(L.DD_X0_DYNAMIC if threshold.mode == "dynamic" else L.DD_X0_STATIC, float(threshold.quantile),
                             float(threshold.range), float(threshold.s_max))


def _known_region(region, x, n_steps):
    """A KnownRegion as the loops' entries take it: the checks of its tensors against x and of its n_steps (ka, kb) rows, a byref of the
    dd_known_region, and the row arrays, which must outlive the call (a byref keeps its struct alive).  None: (None, None)."""
    if region is None:
        return None, None
    B, Cc, S, _ = x.shape
    for v, shape in ((region.x0, (B, Cc, S, S)), (region.mask, (B, 1, S, S))):
        assert v.is_cuda and v.dtype == torch.float32 and v.is_contiguous() and tuple(v.shape) == shape
    ka, kb = keep = [np.ascontiguousarray(v, np.float32) for v in (region.ka, region.kb)]
    assert ka.shape == kb.shape == (n_steps,)
    kr = L.dd_known_region(region.x0.data_ptr(), region.mask.data_ptr(), *(v.ctypes.data_as(C.POINTER(C.c_float)) for v in keep))
    return C.byref(kr), keep


def _guidance_refs(guidance):
    """A loop's `guidance` value (None, (scale, null_label) or Autoguidance) as the entries' (dd_guidance, dd_autoguidance) byrefs, at most
    one of them set (a byref keeps its struct alive)."""
    if isinstance(guidance, Autoguidance):
        return None, C.byref(L.dd_autoguidance(guidance.guide.handle, float(guidance.scale)))
    return (C.byref(guidance_struct(guidance)) if guidance is not None else None), None


def _loop_call(ctx, args, plain, guidance, region, x, threshold=None):
    """The loop entry of this argument struct as call(stream): `plain` (guidance None), its _guided form (guidance = (scale, null_label):
    classifier-free), its _autoguided form (guidance = Autoguidance(guide, scale)) or, with a KnownRegion, its _region form, which
    takes either kind of guidance, or none, beside the dd_known_region.  guidance = Perturbed(scale, layers_first, layers_late): its
    _perturbed form, alone.  No entry takes two kinds of guidance."""
    if isinstance(guidance, Perturbed):
        if region is not None or threshold is not None:
            raise ValueError("perturbed-attention guidance does not combine with a known region or x0 thresholding")
        pag = L.dd_pag(float(guidance.scale), layer_mask(guidance.layers_first), layer_mask(guidance.layers_late))
        fn = getattr(ctx.lib, plain + "_perturbed")
        return lambda st: fn(ctx.handle, C.byref(args), C.byref(pag), st)
    g, ag = _guidance_refs(guidance)
    kr, keep = _known_region(region, x, args.n_steps if hasattr(args, "n_steps") else args.t_start - args.t_end + 1)
    if region is None and threshold is None:
        name, extra = plain + ("" if guidance is None else "_autoguided" if g is None else "_guided"), [r for r in (g, ag) if r is not None]
    elif threshold is None:
        name, extra = plain + "_region", [g, ag, kr]
    else:
        name, extra = plain + "_threshold", [g, ag, kr, C.byref(threshold_struct(threshold))]
    fn = getattr(ctx.lib, name)
    return lambda st, keep=keep: fn(ctx.handle, C.byref(args), *extra, st)     # (a byref keeps its struct alive, the closure the arrays)


def _run_loop(ctx: Context, args, x, y, seed, noise, use_graph, stream, call, image="x_dev"):
    """Fill the fields every loop's argument struct shares (x in place, y, the device noise) and run call(stream) on the caller's stream.
    image: the field that receives x's pointer (the scans only read their images: x0_dev)."""
    args.noise_mode = {"none": L.DD_NOISE_NONE, "philox": L.DD_NOISE_PHILOX}[noise]
    args.use_graph = int(bool(use_graph))
    args.seed = int(seed)
    args.y_dev = y.data_ptr() if y is not None else None
    setattr(args, image, x.data_ptr())
    args.B = x.shape[0]
    cur = stream if stream is not None else torch.cuda.current_stream(x.device)
    if use_graph and cur.cuda_stream == 0:
        # hipGraph capture is not permitted on the legacy default stream: run the loop on a private side stream, ordered
        # after the caller's work and before whatever the caller enqueues next
        side = ctx.side_stream(x.device)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            ctx.check(call(_stream_ptr(side)))
        cur.wait_stream(side)
    else:
        ctx.check(call(_stream_ptr(cur)))
    return x


def sample_loop(ctx: Context, first: Model, late, x, *, t_switch=0, t_start=999, t_end=0, y=None, seed=0,
                noise="philox", variance="beta_tilde", use_graph=True, stream=None, guidance=None):
    """dd_sample: the whole DDPM loop on the device (hipGraph replay per backbone), in place on x.
    guidance = (scale, null_label): classifier-free guidance (dd_sample_guided; labels y required, max_batch >= 2 B);
    guidance = Autoguidance(guide_model, scale): autoguidance (dd_sample_autoguided)."""
    return _sample_loop(ctx, first, late, x, None, t_switch, t_start, t_end, y, seed, noise, variance, use_graph, stream, guidance)


def sample_region_loop(ctx: Context, first: Model, late, x, region: KnownRegion, *, t_switch=0, t_start=999, t_end=0, y=None, seed=0,
                       noise="philox", variance="beta_tilde", use_graph=True, stream=None, guidance=None):
    """dd_sample_region: sample_loop with a known region; region.ka / kb hold t_start - t_end + 1 rows, row k the step at t_start - k."""
    return _sample_loop(ctx, first, late, x, region, t_switch, t_start, t_end, y, seed, noise, variance, use_graph, stream, guidance)


def _sample_loop(ctx, first, late, x, region, t_switch, t_start, t_end, y, seed, noise, variance, use_graph, stream, guidance):
    args = L.dd_sample_args()
    args.first = first.handle
    args.late = late.handle if late is not None else None
    args.t_switch = int(t_switch) if t_switch and np.isfinite(t_switch) else 0
    args.t_start, args.t_end = int(t_start), int(t_end)
    args.variance = L.DD_VAR_BETA if variance == "beta" else L.DD_VAR_BETA_TILDE
    return _run_loop(ctx, args, x, y, seed, noise, use_graph, stream, _loop_call(ctx, args, "dd_sample", guidance, region, x))


def _step_table(args, first, late, rows, floats, ints, switch_after, counter_base):
    """Fill the fields dd_sample_affine's and dd_sample_multistep's argument structs share: the models, the switch, the Philox counter
    base and the step table, rows[k] for k in floats as float32 and in ints as int32, one value per step.  Returns the arrays, which
    must outlive the call."""
    tab = {k: np.ascontiguousarray(rows[k], np.float32) for k in floats}
    tab.update((k, np.ascontiguousarray(rows[k], np.int32)) for k in ints)
    n = len(rows["t"])
    assert all(v.shape == (n,) for v in tab.values())
    for k, v in tab.items():
        setattr(args, k, v.ctypes.data_as(C.POINTER(C.c_float if v.dtype == np.float32 else C.c_int32)))
    args.first = first.handle
    args.late = late.handle if late is not None else None
    args.n_steps = n
    args.switch_after = n if (late is None or switch_after is None) else int(switch_after)
    args.counter_base = int(counter_base)
    return tab


def sample_affine_loop(ctx: Context, first: Model, late, x, t, a, b, c, noise_flags, *, switch_after=None, y=None, seed=0,
                       counter_base=0, noise="philox", use_graph=True, stream=None, guidance=None):
    """dd_sample_affine: the table-driven loops (DDIM, predict_original / predict_previous) on the device, in place on x:
    x <- a[k] x + b[k] model(x, t[k]) + c[k] z for k = 0 .. len(t) - 1; the late model runs from step switch_after on.
    Step k draws z from Philox(key = seed, counter = counter_base + k): a loop cut into several calls passes the number
    of steps already done as counter_base and draws exactly the z of the uncut loop.
    guidance = (scale, null_label): classifier-free guidance of the model output (dd_sample_affine_guided);
    guidance = Autoguidance(guide_model, scale): autoguidance of it (dd_sample_affine_autoguided)."""
    return _sample_affine_loop(ctx, first, late, x, None, t, a, b, c, noise_flags, switch_after, y, seed, counter_base, noise, use_graph,
                               stream, guidance)


def sample_affine_region_loop(ctx: Context, first: Model, late, x, region: KnownRegion, t, a, b, c, noise_flags, *, switch_after=None,
                              y=None, seed=0, counter_base=0, noise="philox", use_graph=True, stream=None, guidance=None):
    """dd_sample_affine_region: sample_affine_loop with a known region; region.ka / kb hold one row per step of the call."""
    return _sample_affine_loop(ctx, first, late, x, region, t, a, b, c, noise_flags, switch_after, y, seed, counter_base, noise,
                               use_graph, stream, guidance)


def _sample_affine_loop(ctx, first, late, x, region, t, a, b, c, noise_flags, switch_after, y, seed, counter_base, noise, use_graph,
                        stream, guidance):
    args = L.dd_affine_sample_args()
    tab = _step_table(args, first, late, dict(t=t, a=a, b=b, c=c, noise=noise_flags), "tabc", ("noise",), switch_after,  # noqa: F841
                      counter_base)
    return _run_loop(ctx, args, x, y, seed, noise, use_graph, stream, _loop_call(ctx, args, "dd_sample_affine", guidance, region, x))


def sample_affine_walk_loop(ctx: Context, first: Model, late, x, rows, *, region=None, guidance=None, switch_after=None, y=None, seed=0,
                            counter_base=0, noise="philox", use_graph=True, stream=None):
    """dd_sample_affine_walk: sample_affine_loop over a walk that may go back up (RePaint's resampling, Restart sampling), in place on x.
    rows: a dict with t, a, b, c, noise, jump and optionally late (a walk plan's rows, step_plan.step_plan(..., resample_jump= ...), or any
    slice of them).  Row k with jump[k] == 0 is sample_affine_loop's step, run by the late model where late[k] == 1 (no late row: from
    row switch_after on); with jump[k] != 0 it runs no model: x <- a[k] x + c[k] z3, z3 a Philox draw of its own stream under the row's
    counter counter_base + k.  region: a KnownRegion with one (ka, kb) per row (a jump's is not read); guidance: (scale, null_label) or
    Autoguidance(guide_model, scale)."""
    if isinstance(guidance, Perturbed):
        raise ValueError("perturbed-attention guidance does not combine with resampling jumps")
    args = L.dd_affine_sample_args()
    tab = _step_table(args, first, late, rows, "tabc", ("noise",), switch_after, counter_base)
    n = args.n_steps
    prog = [np.ascontiguousarray(rows[k], np.int32) if k in rows and rows[k] is not None else None for k in ("jump", "late")]
    assert prog[0] is not None and all(v is None or v.shape == (n,) for v in prog)
    walk = L.dd_walk(*(v.ctypes.data_as(C.POINTER(C.c_int32)) if v is not None else None for v in prog))
    (g, ag), (kr, keep) = _guidance_refs(guidance), _known_region(region, x, n)
    # (a byref keeps its struct alive, the closure the arrays)
    call = lambda st, keep=(tab, prog, keep): ctx.lib.dd_sample_affine_walk(ctx.handle, C.byref(args), g, ag, kr, C.byref(walk), st)
    return _run_loop(ctx, args, x, y, seed, noise, use_graph, stream, call)


def sample_affine_cached_loop(ctx: Context, first: Model, late, x, rows, *, blocks, order=0, region=None, guidance=None, switch_after=None,
                              y=None, seed=0, counter_base=0, noise="philox", use_graph=True, stream=None):
    """dd_sample_affine_cached: sample_affine_loop with block caching, in place on x.  rows: a dict with t, a, b, c, noise, cache and cw (a
    cached plan's rows, step_plan.step_plan(..., cache_blocks= ...), or any slice of them): row k with cache[k] == 0 is a refresh step of
    its model (the full forward, which stores the output of the deep blocks `blocks` .. depth - 1 - blocks), with cache[k] == 1 a reuse
    step (those blocks do not run) and with cache[k] == 2 (order 1 only) a reuse step on the extrapolation last + cw[k] (last - prev).
    What a model's cache holds outlives the call: a loop cut at any row continues where the uncut loop would.  region: a KnownRegion
    with one (ka, kb) per row; guidance: (scale, null_label), classifier-free, or None."""
    if guidance is not None and (isinstance(guidance, (Perturbed, Autoguidance)) or len(guidance) != 2):
        raise ValueError("block caching combines with classifier-free guidance only")
    args = L.dd_affine_sample_args()
    tab = _step_table(args, first, late, rows, "tabc", ("noise",), switch_after, counter_base)
    n = args.n_steps
    keep = [np.ascontiguousarray(rows["cache"], np.int32), np.ascontiguousarray(rows["cw"], np.float32)]
    assert all(v.shape == (n,) for v in keep)
    bc = L.dd_block_cache(int(blocks), int(order), keep[0].ctypes.data_as(C.POINTER(C.c_int32)), keep[1].ctypes.data_as(C.POINTER(C.c_float)))
    (g, _), (kr, kab) = _guidance_refs(guidance), _known_region(region, x, n)
    # (a byref keeps its struct alive, the closure the arrays)
    call = lambda st, keep=(tab, keep, kab): ctx.lib.dd_sample_affine_cached(ctx.handle, C.byref(args), g, kr, C.byref(bc), st)
    return _run_loop(ctx, args, x, y, seed, noise, use_graph, stream, call)


def sample_multistep_loop(ctx: Context, first: Model, late, x, h, rows, *, switch_after=None, y=None, seed=0, counter_base=0,
                          noise="philox", use_graph=True, stream=None, guidance=None):
    """dd_sample_multistep: the DPM-Solver++ loop on the device, in place on x and on its history register h (same shape as x):
    x <- a[k] x + b[k] m_k [+ d[k] h if hist[k]] [+ c[k] z if noise[k]], h <- p[k] x + q[k] m_k for k = 0 .. len(t) - 1, m_k the
    model output at t[k].  rows: a dict with t, a, b, c, d, p, q, noise, hist (sampler.multistep_coefficients, or any slice of it).
    The late model runs from step switch_after on; Philox counters as sample_affine_loop.  A loop cut into several calls passes h on.
    guidance = (scale, null_label): classifier-free guidance of the model output (dd_sample_multistep_guided);
    guidance = Autoguidance(guide_model, scale): autoguidance of it (dd_sample_multistep_autoguided)."""
    return _sample_multistep_loop(ctx, first, late, x, None, h, rows, switch_after, y, seed, counter_base, noise, use_graph, stream,
                                  guidance)


def sample_multistep_region_loop(ctx: Context, first: Model, late, x, region: KnownRegion, h, rows, *, switch_after=None, y=None,
                                 seed=0, counter_base=0, noise="philox", use_graph=True, stream=None, guidance=None):
    """dd_sample_multistep_region: sample_multistep_loop with a known region (h is not touched by it); region.ka / kb hold one row per
    step of the call."""
    return _sample_multistep_loop(ctx, first, late, x, region, h, rows, switch_after, y, seed, counter_base, noise, use_graph, stream,
                                  guidance)


def sample_multistep_threshold_loop(ctx: Context, first: Model, late, x, h, rows, threshold: X0Threshold, *, region=None, switch_after=None,
                                    y=None, seed=0, counter_base=0, noise="philox", use_graph=True, stream=None, guidance=None):
    """dd_sample_multistep_threshold: sample_multistep_loop on UNFOLDED rows (sampler.multistep_coefficients(..., unfolded=True) and its
    DDIM / DDPM forms) with every step's data prediction x0 = p[k] x + q[k] m_k thresholded: x <- a[k] x + b[k] xh [+ d[k] h] [+ c[k] z],
    h <- xh.  region (a KnownRegion) and guidance are optional, as in the other loops."""
    return _sample_multistep_loop(ctx, first, late, x, region, h, rows, switch_after, y, seed, counter_base, noise, use_graph, stream,
                                  guidance, threshold)


def _sample_multistep_loop(ctx, first, late, x, region, h, rows, switch_after, y, seed, counter_base, noise, use_graph, stream, guidance,
                           threshold=None):
    args = L.dd_multistep_sample_args()
    tab = _step_table(args, first, late, rows, "tabcdpq", ("noise", "hist"), switch_after, counter_base)  # noqa: F841
    assert h.is_cuda and h.dtype == torch.float32 and h.is_contiguous() and h.shape == x.shape
    args.h_dev = h.data_ptr()
    return _run_loop(ctx, args, x, y, seed, noise, use_graph, stream, _loop_call(ctx, args, "dd_sample_multistep", guidance, region, x, threshold))


def _ee_sample_args(model, x, threshold, t_start, t_end, err, idx):
    """The dd_ee_sample_args of the two early-exit loops: the fields of their own, and the checks of the two log tables (each may be None)"""
    args = L.dd_ee_sample_args()
    args.model = model.handle
    args.threshold = float(threshold)
    args.t_start, args.t_end = int(t_start), int(t_end)
    if err is not None:
        assert err.is_cuda and err.dtype == torch.float32 and err.is_contiguous() and err.shape[0] == 1000
    if idx is not None:
        assert idx.is_cuda and idx.dtype == torch.int32 and idx.is_contiguous() and tuple(idx.shape) == (1000, x.shape[0])
    args.err_dev = err.data_ptr() if err is not None else None
    args.idx_dev = idx.data_ptr() if idx is not None else None
    return args


def sample_early_exit_loop(ctx: Context, model: Model, x, threshold, *, t_start=999, t_end=0, y=None, seed=0, noise="philox",
                           err=None, idx=None, use_graph=True, stream=None):
    """dd_sample_early_exit: the early-exit baseline's loop (eesampler.py:40-89) on the device, in place on x.
    err [1000, depth] fp32 / idx [1000, B] int32 device tensors (or None): rows t_start .. t_end are written."""
    args = _ee_sample_args(model, x, threshold, t_start, t_end, err, idx)
    call = lambda st: ctx.lib.dd_sample_early_exit(ctx.handle, C.byref(args), st)
    return _run_loop(ctx, args, x, y, seed, noise, use_graph, stream, call)


def sample_early_exit_real_loop(ctx: Context, model: Model, x, threshold, *, t_start=999, t_end=0, y=None, seed=0, noise="philox",
                                idx=None, compact_every=1, err=None, stream=None):
    """dd_sample_early_exit_real: sample_early_exit_loop with the exits taken -- an image that has left runs no block from the next
    compaction layer (every compact_every-th, from layer 0) on.  Images and idx rows equal sample_early_exit_loop's bit for bit.  The
    loop runs as eager launches and blocks the calling thread: the host waits for the active count at every compaction layer; no graph
    is captured or replayed.  err must be None (the batch mean of a layer's predicted errors does not exist once images have left).
    Returns x; real_exit_stats(ctx) reports what the call ran."""
    if err is not None:
        raise ValueError("real early exit writes no error_prediction_by_timestep: err must be None")
    if int(compact_every) != compact_every or int(compact_every) < 1:
        raise ValueError(f"compact_every must be an integer >= 1, got {compact_every!r}")
    if noise not in ("none", "philox"):
        raise ValueError("real early exit draws its noise on the device: noise must be 'philox' or 'none'")
    args = _ee_sample_args(model, x, threshold, t_start, t_end, None, idx)
    real = L.dd_ee_real(int(compact_every), 0)
    call = lambda st: ctx.lib.dd_sample_early_exit_real(ctx.handle, C.byref(args), C.byref(real), st)
    return _run_loop(ctx, args, x, y, seed, noise, False, stream, call)


def real_exit_stats(ctx: Context):
    """dd_dev_ee_real_stats of the last sample_early_exit_real_loop call: (block-rows run, moves made, compactions made)."""
    out = (C.c_longlong * 3)()
    ctx.check(ctx.lib.dd_dev_ee_real_stats(ctx.handle, out))
    return tuple(int(v) for v in out)


def _scan_args(args, model, rows, counter_base):
    """The fields dd_scan_args and dd_scan_exits_args share, from the six row arrays (kept alive on args as float32); returns n."""
    args._rows = {k: np.ascontiguousarray(rows[k], np.float32) for k in ("t", "ka", "kb", "tz", "t0", "tx")}
    n = len(args._rows["t"])
    assert all(v.shape == (n,) for v in args._rows.values())
    for k, v in args._rows.items():
        setattr(args, k, v.ctypes.data_as(C.POINTER(C.c_float)))
    args.model = model.handle
    args.n_steps = n
    args.counter_base = int(counter_base)
    return n


def scan_error_loop(ctx: Context, model: Model, x0, rows, *, y=None, seed=0, counter_base=0, err=None, use_graph=True, stream=None):
    """dd_scan_error: the denoising error of `model` on the images x0 [B, C, S, S] (model space; only read) at every row of `rows`
    (step_plan.scan_rows, or any slice of it): step k noises the images to x_t = ka[k] x0 + kb[k] z with the image's own Philox draw
    (counter counter_base + k, a stream word of its own; per-image seeds are honoured), runs the model at t[k] and writes
    err[k, i] = mean((model(x_t) - (tz[k] z + t0[k] x0 + tx[k] x_t))^2) over image i.  One device-resident loop, graph replays and
    half-batch chains as sample_loop.  Returns err [n, B] fp32 on the device.  Two models called with the same x0, seed (or image
    seeds) and counter_base see the same (x0, z, t): a paired comparison."""
    assert x0.is_cuda and x0.dtype == torch.float32 and x0.is_contiguous() and x0.dim() == 4
    args = L.dd_scan_args()
    n = _scan_args(args, model, rows, counter_base)
    err = torch.empty(n, x0.shape[0], device=x0.device, dtype=torch.float32) if err is None else err
    assert err.is_cuda and err.dtype == torch.float32 and err.is_contiguous() and tuple(err.shape) == (n, x0.shape[0])
    args.err_dev = err.data_ptr()
    _run_loop(ctx, args, x0, y, seed, "philox", use_graph, stream, lambda st: ctx.lib.dd_scan_error(ctx.handle, C.byref(args), st),
              image="x0_dev")
    return err


def scan_exits_loop(ctx: Context, model: Model, x0, rows, *, y=None, seed=0, counter_base=0, use_graph=True, stream=None):
    """dd_scan_error_early_exit: scan_error_loop for an early-exit model -- from the one forward of step k every exit's error.  rows as
    scan_error_loop, their t distinct integers in [0, 999].  Returns (mse [n, depth + 1, B], target [n, depth + 1, B], pred [n, depth, B])
    fp32 on the device: exit l < depth is the head behind block l, exit depth the backbone; mse as scan_error_loop's err, target the
    mean of tanh|output - training target| (what probe l was trained to predict), pred the probes' predictions (what the early-exit
    sampler compares with --threshold)."""
    assert x0.is_cuda and x0.dtype == torch.float32 and x0.is_contiguous() and x0.dim() == 4
    args = L.dd_scan_exits_args()
    n = _scan_args(args, model, rows, counter_base)
    B, depth = x0.shape[0], model.mp.depth
    mse, target = (torch.empty(n, depth + 1, B, device=x0.device, dtype=torch.float32) for _ in range(2))
    pred = torch.empty(n, depth, B, device=x0.device, dtype=torch.float32)
    args.mse_dev, args.target_dev, args.pred_dev = mse.data_ptr(), target.data_ptr(), pred.data_ptr()
    _run_loop(ctx, args, x0, y, seed, "philox", use_graph, stream, lambda st: ctx.lib.dd_scan_error_early_exit(ctx.handle, C.byref(args), st),
              image="x0_dev")
    return mse, target, pred
