"""DuoDiff sampling driver: the reference's ``sampler.py`` surface on the MI355X engine.

Same command line (reference sampler.py:192-252), YAML configs and checkpoint formats; the
1000-step loop of ``get_samples`` (sampler.py:82-155) runs as fused HIP steps -- either one
hipGraph replay per step entirely on the device (``--noise device``), or step by step with z
drawn from the torch CPU stream exactly as the reference draws it (``--noise torch_cpu``,
bit-identical noise for parity runs).

    python -m duodiff_amd.sampler --config_path configs/uvit_celeba_3.yaml --checkpoint_path s.pth \
        --config_path_late configs/uvit_celeba.yaml --checkpoint_path_late f.pth --t_switch 300 \
        --batch_size 128 --parametrization predict_noise --output_folder out

DDIM (--use_ddim) and the predict_original / predict_previous parametrizations run
the U-ViT forward on the engine plus one fused affine update per step; ImageNet-256 latents are decoded by the
engine's KL-VAE decoder when the YAML carries an ``autoencoder`` block (next-1).

Classifier-free guidance (engine option, not in the reference): ``--cfg_scale 0.4 --class_label 207`` samples a class-conditional
model with eps = eps_c + s (eps_c - eps_u), the unconditional rows labelled ``--cfg_null_label`` (U-ViT's null class 1000), the
combination fused into the step kernel of every loop.

Autoguidance (engine option, not in the reference): ``--autoguidance_scale 1.0`` on a DuoDiff run (``--checkpoint_path_late``) guides
every step of the full model with the shallow one, eps = eps_full + s (eps_full - eps_shallow), both backbones on the same rows and the
combination fused into the step kernel; the shallow model's own steps stay unguided.  ``--guide_config_path`` / ``--guide_checkpoint_path``
name an explicit guide for a single-backbone run.  No labels are needed: unconditional models can be guided.

Perturbed-attention guidance (engine option, not in the reference; Ahn et al. 2024): ``--pag_scale 3.0`` guides ONE model, unconditional
ones included, with itself: every step also evaluates it with the self-attention map of the blocks ``--pag_layers`` (default: the middle
block) replaced by the identity and uses eps = eps + s (eps - eps_perturbed), fused into the step kernel of every loop.

Image-to-image and inpainting (engine options, not in the reference): ``--init_image x.npy --strength 0.5`` starts every loop from the
given image noised to t = round(999 * 0.5) instead of from pure noise (SDEdit; latent models: .npy latents, or pixel-space files with
``--encode_images``, which the KL-VAE encoder of the engine turns into latents); ``--known_image x.npy --known_mask m.npy`` keeps the
masked region of the image fixed while the rest is generated (RePaint's replacement rule without resampling), fused into the step kernel.

Resampling jumps (engine options, not in the reference): ``--resample_jump 10 --resample_count 10`` walks the DDPM / DDIM grid with
RePaint's schedule (Lugmayr et al. 2022): every 10 grid steps x is noised back up 10 steps and brought down again, 10 times in all, so that
the generated region of an inpainting run (``--known_image``) can agree with the known one; ``--restart T_MIN T_MAX K`` (repeatable) is
Restart sampling (Xu et al. 2023): K returns from the level T_MIN up to T_MAX.  A jump runs no model; the whole walk is one device loop.

Block caching (engine option, not in the reference; DeepCache, Ma et al. 2024): ``--cache_blocks 2 --cache_interval 3`` runs the full
backbone on every third step of a model only; the steps between run its two outermost blocks on either side and feed the long skip
path the deep blocks' output of the last full step (``--cache_order 1``: a linear extrapolation of the last two, TaylorSeer).  DDPM and
DDIM loops, with classifier-free guidance, a known region, an init image, image seeds and a late model; training-free, on any checkpoint.

DPM-Solver++ (engine option, not in the reference): ``--dpm_solver ode --dpm_solver_steps 20`` samples with the second-order multistep
solver (``sde``: its SDE variant) in 20 model evaluations; the table-driven loop with one history register per image.
"""
import contextlib
import math
import random
import time
from argparse import ArgumentParser
from collections import namedtuple
from pathlib import Path
from typing import List

import numpy as np
import torch

from .config import ModelParams, load_config
from .autoencoder import get_autoencoder
from .engine import (Autoguidance, Context, KnownRegion, Perturbed, X0Threshold, layer_mask, sample_affine_loop, sample_affine_region_loop,
                     sample_affine_cached_loop, sample_affine_walk_loop, sample_loop,
                     sample_multistep_loop, sample_multistep_region_loop, sample_multistep_threshold_loop, sample_region_loop,
                     schedule_tables, threshold_struct)
from .step_plan import (MULTISTEP_KINDS, StepPlan, _affine_rows, _data_prediction, _f32, _segments, affine_coefficients, known_rows,  # noqa: F401
                        jump_coefficients, multistep_coefficients, multistep_grid, multistep_rows, repaint_jumps, restart_jumps, start_timestep,
                        cache_rows, step_plan, unfolded_coefficients, unfolded_rows, cache_settings, walk_moves)
from .uvit import UViT


def get_device():
    """reference sampler.py:25-38 picks cuda:0 > mps > cpu; this engine exists only for the GPU."""
    if not torch.cuda.is_available():
        raise RuntimeError("duodiff_amd needs an MI355X GPU; there is no CPU sampling path")
    return f"cuda:{torch.cuda.current_device()}"


def seed_everything(seed):
    """reference utils/train_utils.py:8-12."""
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed(seed)
    random.seed(seed)
    np.random.seed(seed)


class _Schedule:
    """Module-level tables of reference sampler.py:40-44, materialised lazily from the engine."""

    def __getattr__(self, name):
        t = schedule_tables()
        self.betas = torch.from_numpy(t["betas"].copy())
        self.alphas = torch.from_numpy(t["alphas"].copy())
        self.alphas_bar = torch.from_numpy(t["alphas_bar"].copy())
        self.alphas_bar_previous = torch.from_numpy(t["alphas_bar_previous"].copy())
        self.betas_tilde = torch.from_numpy(t["betas_tilde"].copy())
        if name in self.__dict__:
            return self.__dict__[name]
        raise AttributeError(name)


schedule = _Schedule()


def predict_noise_postprocessing(model_output, x, t, z=None):
    """reference sampler.py:47-56 on device tensors.  ``z``: the noise to use (default: drawn from
    the torch CPU stream, like ``randn_like`` on a CPU reference run); ignored at t == 0."""
    ctx = Context.get(x.device)
    if t > 0 and z is None:
        z = torch.randn(x.shape).to(x.device)
    return ctx.ddpm_step(x.contiguous(), model_output, z if t > 0 else None, t)


def _affine_post(kind, model_output, x, t, z=None):
    ctx = Context.get(x.device)
    a, b, c = affine_coefficients(kind, t)
    if t > 0 and z is None:
        z = torch.randn(x.shape).to(x.device)          # randn_like on the torch CPU stream (sampler.py:67,77)
    return ctx.affine_step(x, model_output, z if t > 0 else None, a, b, c)


def predict_original_postprocessing(model_output, x, t, z=None):
    """reference sampler.py:59-72 (model predicts x_0) on device tensors."""
    return _affine_post("predict_original", model_output, x, t, z)


def predict_previous_postprocessing(model_output, x, t, z=None):
    """reference sampler.py:75-79 (model predicts x_{t-1}) on device tensors."""
    return _affine_post("predict_previous", model_output, x, t, z)


_PARAMETRIZATIONS = {predict_noise_postprocessing: "predict_noise", predict_original_postprocessing: "predict_original",
                     predict_previous_postprocessing: "predict_previous"}


def _batch_tensor(v, name, batch_size, shape, device):
    """An image argument of get_samples as a contiguous fp32 device tensor [B, *shape]; a leading 1 is repeated over the batch"""
    t = torch.as_tensor(np.asarray(v.detach().cpu()) if isinstance(v, torch.Tensor) else np.asarray(v), dtype=torch.float32)
    if t.dim() != 4 or t.shape[0] not in (1, batch_size) or tuple(t.shape[1:]) != tuple(shape):
        raise ValueError(f"{name} must have shape [1 or {batch_size}, {', '.join(map(str, shape))}], not {list(t.shape)}")
    return t.expand(batch_size, *shape).contiguous().to(device)


def backbone_rows(batch_size, cfg_scale=None, pag=None):
    """Backbone rows per step (a model's max_batch): 2 B with the unconditional / perturbed half of CFG or PAG, else B (autoguidance too)"""
    return 2 * batch_size if cfg_scale is not None or pag is not None else batch_size


def _resolve_options(model, late_model, batch_size, image_shape, plan_args, noise, y, autoencoder, cfg_scale, cfg_null_label,
                     autoguidance_scale, guide_model, pag, image_seeds, init_image, strength, known_image, known_mask, threshold, walk=False,
                     cache=None):
    """get_samples' one options check, before any engine call: every ValueError it raises, in a fixed order.  Returns the StepPlan of
    plan_args; the run's ONE guidance, which the device loops take and the host step picks its forward call by -- None, (scale, null_label),
    Autoguidance(the guide's UViT, scale) or Perturbed(scale, mask_first, mask_late); the seeds as ints; the init image and KnownRegion."""
    if noise not in ("torch_cpu", "device"):
        raise ValueError("noise must be 'torch_cpu' or 'device'")
    guidance = None
    if autoguidance_scale is not None:
        if cfg_scale is not None:
            raise ValueError("classifier-free guidance and autoguidance are exclusive")
        if not math.isfinite(float(autoguidance_scale)):
            raise ValueError("autoguidance_scale must be finite")
        if guide_model is None and late_model is None:
            raise ValueError("autoguidance needs a guide model: pass guide_model, or a late_model (the first model then guides it)")
        guidance = Autoguidance(model if guide_model is None else guide_model, float(autoguidance_scale))
    elif guide_model is not None:
        raise ValueError("guide_model without autoguidance_scale")
    if pag is not None:
        if cfg_scale is not None or autoguidance_scale is not None or known_image is not None or init_image is not None or threshold is not None:
            raise ValueError("perturbed-attention guidance does not combine with classifier-free guidance, autoguidance, a known region, "
                             "an init image or x0 thresholding")
        guidance = Perturbed(float(pag[0]), layer_mask(pag[1]), layer_mask(pag[2] if len(pag) > 2 else 0))
        if not math.isfinite(guidance.scale):
            raise ValueError("pag scale must be finite")
        for mdl, mask, what in ((model, guidance.layers_first, "layers_first"), (late_model, guidance.layers_late, "layers_late")):
            if mdl is not None and mask >> mdl.depth:
                raise ValueError(f"pag {what} names a block at or above the model's depth {mdl.depth}")
    if image_seeds is not None:
        if noise != "device":
            raise ValueError("image_seeds need noise='device': the torch CPU stream is sequential in the batch")
        image_seeds = [int(v) for v in image_seeds]
        if len(image_seeds) != batch_size:
            raise ValueError(f"image_seeds holds {len(image_seeds)} seeds for batch_size {batch_size}")
    if walk:
        if pag is not None:
            raise ValueError("perturbed-attention guidance does not combine with resampling jumps (resample_jump / restart)")
        if any(hasattr(m, "classifier_type") for m in (model, late_model) if m is not None):
            raise ValueError("resampling jumps are not supported for early-exit models")
    if cache is not None:
        if pag is not None or autoguidance_scale is not None:
            raise ValueError("block caching does not combine with perturbed-attention guidance or autoguidance")
        if any(hasattr(m, "classifier_type") for m in (model, late_model) if m is not None):
            raise ValueError("block caching is not supported for early-exit models")
        cache_settings(*cache, depths=[m.depth for m in (model, late_model) if m is not None])
    if (init_image is None) != (strength is None):
        raise ValueError("init_image and strength go together")
    if (known_image is None) != (known_mask is None):
        raise ValueError("known_image and known_mask go together")
    plan = step_plan(*plan_args)
    if threshold is not None:
        if autoencoder is not None:
            raise ValueError("x0 thresholding is for pixel-space models: a latent model's x0 is a latent, not an image in [-1, 1]")
        threshold_struct(threshold)
    if cfg_scale is not None:
        guidance = (float(cfg_scale), int(cfg_null_label))
        if y is None:
            raise ValueError("classifier-free guidance needs class labels")
    init = None if init_image is None else _batch_tensor(init_image, "init_image", batch_size, image_shape, model.device)
    region = None
    if known_image is not None:
        mask = _batch_tensor(known_mask, "known_mask", batch_size, (1,) + image_shape[1:], model.device)
        if not bool(((mask >= 0) & (mask <= 1)).all()):
            raise ValueError("known_mask must lie in [0, 1]")
        region = KnownRegion(_batch_tensor(known_image, "known_image", batch_size, image_shape, model.device), mask, *known_rows(plan))
    return plan, guidance, image_seeds, init, region


def _start(ctx, device, batch_size, image_shape, seed, image_seeds, init, t0):
    """x_T from the torch CPU stream after seed_everything(seed) (sampler.py:99-100), or image i on the device under image_seeds[i];
    with an init image (t0 < 999): x_t0 = sqrt(abar) init + sqrt(1 - abar) x_T."""
    seed_everything(seed)
    if image_seeds is None:
        x = torch.randn(batch_size, *image_shape).to(device).contiguous()
    elif image_shape[1] != image_shape[2]:
        raise ValueError("image_seeds: square images only")
    else:
        x = ctx.noise_images(batch_size, image_shape[0], image_shape[1], image_seeds=image_seeds, counter=0)
    if t0 < 999:                                                             # (strength 1: t0 = 999, x_T alone)
        ab0 = schedule_tables()["alphas_bar"].astype(np.float64)[t0]
        ctx.affine_step(x, init, None, _f32(np.sqrt(1.0 - ab0)), _f32(np.sqrt(ab0)), 0.0, out=x)
    return x


# what a segment of get_samples works on: the models, x and the solver's history h (updated in place), the host step's eps buffer, the options
_Run = namedtuple("_Run", "ctx plan first late x h eps y guidance threshold region seed use_graph image_seeds cache", defaults=(None,))


def _segment_models(plan, k0, k1, first, late):
    """Who runs the steps [k0, k1) of any plan kind: (the model that starts the segment, the one it switches to inside it or None, the
    first step of that one counted from k0 -- 0: the segment starts behind the switch, k1 - k0: the switch comes later, None: never)"""
    sw = None if plan.switch_after is None else min(max(plan.switch_after - k0, 0), k1 - k0)
    return late if sw == 0 else first, late if sw and sw < k1 - k0 else None, sw


def _device_segment(run, k0, k1):
    """Steps [k0, k1) as one device loop call (hipGraph replays, Philox z) under the run's seed and the Philox counter base k0: cuts do not show"""
    ctx, plan, x, h, tab = run.ctx, run.plan, run.x, run.h, run.plan.rows
    m0, m1, sw = _segment_models(plan, k0, k1, run.first, run.late)
    guidance = run.guidance
    if isinstance(guidance, Perturbed) and sw == 0:                         # m0 is the late model: its blocks are the loop's layers_first
        guidance = guidance._replace(layers_first=guidance.layers_late)
    kw = dict(y=run.y, seed=run.seed, noise="philox", use_graph=run.use_graph, guidance=guidance)
    known = () if run.region is None else (run.region._replace(ka=run.region.ka[k0:k1], kb=run.region.kb[k0:k1]),)   # -> the loop's _region form
    seg = {key: v[k0:k1] for key, v in tab.items()}
    with ctx.image_seeds(run.image_seeds) if run.image_seeds is not None else contextlib.nullcontext():   # (set around the segment's call)
        if plan.moves:              # a walk: the rows name their model, and a jump row runs none
            sample_affine_walk_loop(ctx, run.first, run.late, x, seg, region=known[0] if known else None, counter_base=k0, **kw)
        elif run.cache is not None:  # block caching: the rows name refresh and reuse steps; the models' caches carry over the cuts
            sample_affine_cached_loop(ctx, m0, m1, x, seg, blocks=run.cache[0], order=run.cache[2], region=known[0] if known else None,
                                      switch_after=sw, counter_base=k0, **kw)
        elif plan.kind == "ddpm":   # dd_sample: the late model unless the segment starts on it; t_switch counted from t = 999, not from t[0]
            (sample_region_loop if known else sample_loop)(
                ctx, m0, None if sw == 0 else run.late, x, *known, t_switch=plan.switch_after + 999 - int(tab["t"][0]) if sw else 0,
                t_start=int(seg["t"][0]), t_end=int(seg["t"][-1]), **kw)
        elif plan.kind == "affine":
            (sample_affine_region_loop if known else sample_affine_loop)(
                ctx, m0, m1, x, *known, seg["t"], seg["a"], seg["b"], seg["c"], seg["noise"], switch_after=sw, counter_base=k0, **kw)
        elif run.threshold is not None:
            sample_multistep_threshold_loop(ctx, m0, m1, x, h, seg, run.threshold, region=known[0] if known else None,
                                            switch_after=sw, counter_base=k0, **kw)
        else:
            (sample_multistep_region_loop if known else sample_multistep_loop)(
                ctx, m0, m1, x, *known, h, seg, switch_after=sw, counter_base=k0, **kw)


def _host_step(run, k, k1=None):
    """Step k, the segment [k, k + 1): z, then the known region's z2, from the torch CPU stream in the reference's order (sampler.py:103-139)"""
    ctx, plan, x, h, y, g, eps, tab = run.ctx, run.plan, run.x, run.h, run.y, run.guidance, run.eps, run.plan.rows
    if plan.moves and tab["jump"][k]:                                        # a walk's jump: z3, its one draw; no model, no known blend
        ctx.jump_step(x, torch.randn(x.shape).to(x.device) if tab["noise"][k] else None, tab["a"][k], tab["c"][k], out=x)
        return
    cur, t = _segment_models(plan, k, k + 1, run.first, run.late)[0], tab["t"][k]
    if plan.moves:
        cur = run.late if tab["late"][k] else run.first
    z = torch.randn(x.shape).to(x.device) if tab["noise"][k] else None
    auto = isinstance(g, Autoguidance)
    if plan.kind == "ddpm" and (g is None or auto and g.guide is cur):      # :130-133, fused; the guide's own steps: unguided, y only if it takes one
        cur.sample_step(x, int(t), y=y if not auto or cur.mp.num_classes > 0 else None, z=z, noise="buffer")
    else:
        if run.cache is not None:
            cur.forward_cached(x, float(t), y, blocks=run.cache[0], op=tab["cache"][k], w=tab["cw"][k], guidance=g, out=eps)
        elif g is None:
            cur.forward(x, float(t), y, out=eps)
        elif auto:
            cur.forward_autoguided(x, float(t), y, g.guide, g.scale, out=eps)
        elif isinstance(g, Perturbed):
            cur.forward_perturbed(x, float(t), y, g.scale, g.layers_late if cur is run.late else g.layers_first, out=eps)
        else:
            cur.forward_guided(x, float(t), y, g[0], g[1], out=eps)
        if plan.kind == "ddpm":
            ctx.ddpm_step(x, eps, z, int(t), out=x)
        elif plan.kind == "affine":
            ctx.affine_step(x, eps, z, tab["a"][k], tab["b"][k], tab["c"][k], out=x)
        else:
            thr = () if run.threshold is None else (run.threshold,)
            (ctx.threshold_step if thr else ctx.multistep_step)(x, eps, z, h, *thr, *(tab[key][k] for key in "abcdpq"), tab["hist"][k], out=x)
    if run.region is not None:                                               # z2: its own draw, after the step's z
        z2 = torch.randn(x.shape).to(x.device) if run.region.kb[k] != 0 else None
        ctx.known_blend(x, run.region.x0, run.region.mask, z2, run.region.ka[k], run.region.kb[k], out=x)


def get_samples(model, batch_size: int, postprocessing: callable, seed: int, num_channels: int,
                sample_height: int, sample_width: int, use_ddim: bool = False, ddim_steps: int = 50,
                ddim_eta: float = 0.0, timesteps_save: List[int] = (), y=None, autoencoder=None,
                late_model=None, t_switch=np.inf, *, noise: str = "torch_cpu", use_graph: bool = True,
                num_steps: int = 1000, return_device_tensor: bool = False, cfg_scale=None, cfg_null_label: int = 1000,
                solver=None, solver_steps: int = 20, solver_order: int = 2, autoguidance_scale=None, guide_model=None,
                init_image=None, strength=None, known_image=None, known_mask=None, threshold=None, pag=None, image_seeds=None,
                resample_jump=None, resample_count=None, restart=None, cache=None):
    """reference sampler.py:82-155.  Returns (samples[B,H,W,C] float32 numpy = (x+1)/2, intermediates).

    cfg_scale (None: the unguided loops, unchanged): classifier-free guidance of every step's model output,
        eps_c + cfg_scale * (eps_c - eps_u) with the unconditional rows labelled cfg_null_label; needs labels y.  The backbones run
        2 * batch_size rows (their max_batch grows to that).

    autoguidance_scale (None: off; exclusive with cfg_scale): autoguidance of every step's model output with guide_model (a UViT of the
        same image geometry; default: `model` when a late_model is given, the DuoDiff pair), eps_m + s * (eps_m - eps_guide).  A step
        that guide_model itself runs is the unguided step.  Labels y go to whichever models are class-conditional.

    pag = (scale, layers_first, layers_late) (None: off; exclusive with cfg_scale, autoguidance_scale, known_image, init_image and
        threshold): perturbed-attention guidance of every step's model output, eps + scale * (eps - eps_perturbed), eps_perturbed the
        running model's output with identity attention in its blocks -- layers_first for `model`, layers_late for late_model (block
        indices in forward order, or bit masks).  The backbones run 2 * batch_size rows.  No labels are needed.

    noise="torch_cpu": x_T and every z come from the torch CPU generator after seed_everything(seed),
        in the reference's order -> identical random numbers to a CPU reference run.
    noise="device": x_T as above, z from the device Philox generator inside the graph-replayed loop.
    num_steps < 1000 runs only the first steps (t = 999 ...), for bounded benchmarks.
    image_seeds (None: as above, unchanged; a sequence of batch_size ints; engine option, needs noise="device"): image i depends on
        image_seeds[i] alone, not on its batch -- x_T is drawn on the device (Context.noise_images) and every z and z2 of the loops
        under the image's own seed, so image i equals the batch_size = 1 run with image_seeds = [image_seeds[i]], and a batch equals
        the concatenation of any split of it.  `seed` is then unused by the draws.  (The KL-VAE decode of a latent model is per image
        by construction; nothing is claimed or tested about it here.)

    solver ("dpmsolver++" | "sde-dpmsolver++", engine option, not in the reference): DPM-Solver++ multistep sampling with
        solver_steps model evaluations on the grid multistep_grid(solver_steps) and order solver_order (multistep_coefficients);
        predict_noise or predict_original models.  Step k runs the late model iff t_k < 1000 - t_switch (the DDPM loop's rule).
        Intermediate saves: after the step whose model timestep t has 1000 - t in timesteps_save.

    init_image [1 or B, C, H, W] in the model's own space with strength in (0, 1] (engine option, SDEdit): every loop starts at
        t0 = round(999 * strength) from sqrt(abar[t0]) init_image + sqrt(1 - abar[t0]) z, z the draw x_T is today; strength 1 is the
        present start from z alone.
    known_image [1 or B, C, H, W] with known_mask [1 or B, 1, H, W] in [0, 1] (engine option, inpainting): after every step the pixels
        are finished as mask * (ka known_image + kb z2) + (1 - mask) x' at the noise level the step lands on (known_rows), so the
        result equals known_image where mask == 1.  noise="device": fused into the loops, z2 from the device generator;
        noise="torch_cpu": step by step, z2 drawn from the torch CPU stream after the step's z.
    threshold (an engine.X0Threshold; engine option): every step's predicted image x0 is clipped to a fixed range (mode "static") or to
        its own quantile scale and rescaled (mode "dynamic", Imagen's dynamic thresholding) before it drives the update; all three
        samplers then run as the thresholded multistep loop on unfolded rows.  predict_noise / predict_original models, pixel space.
    resample_jump = j with resample_count = r (engine option; RePaint's resampling), or restart = [(t_min, t_max, K), ...] (engine option;
        Restart sampling): the DDPM / DDIM loop becomes a walk over its grid that also goes back up (step_plan.walk_moves) -- a jump noises x
        forward, x <- ja x + jc z3, and runs no model.  With or without a known region, guidance, image seeds and strength; not with a
        solver, a threshold or pag.  noise="device": one device loop per segment, z3 from the device generator; noise="torch_cpu": step by
        step, a jump's z3 drawn from the torch CPU stream in walk order.  Saves: after the last visit of a saved timestep.
    cache = (K, N, order) (None: every step runs every block, unchanged; engine option; DeepCache): block caching.  Of a model of depth
        2 h + 1 the deep blocks are K .. depth - 1 - K, 1 <= K <= h.  Counted from a model's first step, every N-th step is a refresh: the
        full forward, which stores the deep blocks' output.  The steps between are reuse steps: blocks 0 .. K - 1, then the out-block
        behind the deep range with the stored output (order 0) or with last + w (last - prev), w = (t_1 - t_k) / (t_0 - t_1) from the last
        two refreshes' timesteps (order 1), then on through the head.  The late model starts with a refresh at the switch.  DDPM and DDIM
        loops (the plan is of kind "affine": DDPM on predict_noise runs as table rows); with cfg_scale (the cache holds the 2 B rows), a
        known region, an init image, image seeds and a late model; not with a solver, a threshold, resampling jumps, pag, autoguidance
        or early-exit models.  noise="device": dd_sample_affine_cached; noise="torch_cpu": forward_cached step by step.
    """
    image_shape = (num_channels, sample_height, sample_width)
    plan_args = (_PARAMETRIZATIONS.get(postprocessing), timesteps_save, late_model is not None, t_switch, num_steps, use_ddim, ddim_steps,
                 ddim_eta, solver, solver_steps, solver_order, strength, threshold, resample_jump, resample_count, restart,
                 *(cache if cache is not None else ()))
    plan, guidance, image_seeds, init, region = _resolve_options(
        model, late_model, batch_size, image_shape, plan_args, noise, y, autoencoder, cfg_scale, cfg_null_label, autoguidance_scale,
        guide_model, pag, image_seeds, init_image, strength, known_image, known_mask, threshold,
        walk=resample_jump is not None or resample_count is not None or bool(restart), cache=cache)
    rows = backbone_rows(batch_size, cfg_scale, pag)
    y = None if y is None else torch.as_tensor(y).to(model.device, torch.int64).contiguous()
    first, late = model.engine_model(rows), late_model.engine_model(rows) if late_model is not None else None
    ctx = first.ctx
    x = _start(ctx, model.device, batch_size, image_shape, seed, image_seeds, init, start_timestep(strength))
    if isinstance(guidance, Autoguidance):                                   # the guide's engine model: one of the run's two, or its own
        g = guidance.guide
        guidance = guidance._replace(guide=first if g is model else late if g is late_model else g.engine_model(rows))
    h = torch.zeros_like(x) if plan.kind == "multistep" else None          # the solver's history, carried across save points
    device = noise == "device"
    run = _Run(ctx, plan, first, late, x, h, None if device else torch.empty_like(x), y, guidance, threshold, region, seed, use_graph, image_seeds,
               cache)
    intermediate = []                                                        # (on the host every step is a segment of its own)
    for k0, k1 in _segments(plan.save_after) if device else ((k, k + 1) for k in range(len(plan.save_after))):
        (_device_segment if device else _host_step)(run, k0, k1)
        if plan.save_after[k1 - 1]:
            intermediate.append(x.clone())
    if autoencoder is not None:                                              # the finish: decode (:141-143, :149-150), then the images
        print("Decode the images...")
        x = autoencoder.decode(x)
        intermediate = [autoencoder.decode(v) for v in intermediate]
    samples = ctx.to_images(x.contiguous())                                  # :145-146, library kernel
    inter = [ctx.to_images(v.contiguous()).cpu().numpy() for v in intermediate]
    return (samples if return_device_tensor else samples.cpu().numpy()), inter       # :155 (the D2H boundary)


def draw_labels(batch_size: int, num_classes: int, seeds=None):
    """reference sampler.py:314-318: labels are randint(1, 1001) whatever --class_id says (quirk Q4); a label the embedding
    table does not hold raises the IndexError nn.Embedding raises there (the engine would read past label_emb).
    seeds (per-image seeds): label i is drawn from a generator of its own under seeds[i]."""
    y = torch.randint(1, 1001, (batch_size,)) if seeds is None else torch.cat(
        [torch.randint(1, 1001, (1,), generator=torch.Generator().manual_seed(int(s))) for s in seeds])
    if int(y.max()) >= num_classes or int(y.min()) < 0:
        raise IndexError("index out of range in self")
    return y


def validate_guidance(args, num_classes: int, num_classes_late=None):
    """The label and guidance options against the configs' num_classes, before any GPU work: ValueError on a bad combination."""
    for n in ([num_classes] + ([num_classes_late] if num_classes_late is not None else [])):
        if args.class_label is not None:
            if n <= 0:
                raise ValueError("--class_label needs a class-conditional config (num_classes > 0)")
            if not 0 <= args.class_label < n:
                raise ValueError(f"--class_label {args.class_label} outside [0, {n}) of the config")
        if args.cfg_scale is None:
            continue
        if n <= 0:
            raise ValueError("--cfg_scale needs a class-conditional config (num_classes > 0)")
        if not 0 <= args.cfg_null_label < n:
            raise ValueError(f"--cfg_null_label {args.cfg_null_label} outside [0, {n}): the config has no null-class row to guide against "
                             "(U-ViT's ImageNet-256 layout is num_classes 1001 = 1000 classes + the null label 1000)")
    if args.class_id is not None and args.class_label is not None:
        raise ValueError("--class_id and --class_label are exclusive")
    if args.cfg_scale is not None:
        if not math.isfinite(args.cfg_scale):
            raise ValueError("--cfg_scale must be finite")
        if args.class_id is None and args.class_label is None:
            raise ValueError("--cfg_scale needs class labels: --class_id or --class_label")


def validate_autoguidance(args, config, config_late=None, config_guide=None):
    """The autoguidance options against the YAML configs (the first, the late and the explicit guide's model_params), before any GPU
    work: ValueError on a bad combination."""
    explicit = args.guide_config_path is not None or args.guide_checkpoint_path is not None
    if args.autoguidance_scale is None:
        if explicit:
            raise ValueError("--guide_config_path / --guide_checkpoint_path need --autoguidance_scale")
        return
    if not math.isfinite(args.autoguidance_scale):
        raise ValueError("--autoguidance_scale must be finite")
    if args.cfg_scale is not None:
        raise ValueError("--autoguidance_scale and --cfg_scale are exclusive")
    if explicit and (args.guide_config_path is None or args.guide_checkpoint_path is None):
        raise ValueError("an explicit guide needs both --guide_config_path and --guide_checkpoint_path")
    if not explicit and config_late is None:
        raise ValueError("--autoguidance_scale needs a guide: --checkpoint_path_late (the first model then guides the late one) or "
                         "--guide_config_path / --guide_checkpoint_path")
    guide = ModelParams.from_dict(config_guide if explicit else config)
    for name, cfg in (("--config_path", config), ("--config_path_late", config_late)):
        if cfg is None:
            continue
        mp = ModelParams.from_dict(cfg)
        if (mp.img_size, mp.patch_size, mp.in_chans) != (guide.img_size, guide.patch_size, guide.in_chans):
            raise ValueError(f"autoguidance: the guide's image geometry (img_size, patch_size, in_chans) = "
                             f"{(guide.img_size, guide.patch_size, guide.in_chans)} differs from {name}'s "
                             f"{(mp.img_size, mp.patch_size, mp.in_chans)}")


def pag_layers(spec, depth, what):
    """--pag_layers / --pag_layers_first values (None: the default) -> block indices: "mid" is block depth // 2"""
    spec = ["mid"] if spec is None else spec
    out = []
    for v in spec:
        if v == "mid":
            out.append(depth // 2)
            continue
        try:
            i = int(v)
        except ValueError:
            raise ValueError(f"{what}: 'mid' or block indices, not {v!r}") from None
        if not 0 <= i < depth:
            raise ValueError(f"{what}: block {i} outside [0, {depth}) of the model")
        out.append(i)
    return out


def validate_pag(args, config, config_late=None):
    """The perturbed-attention options against the YAML configs, before any GPU work: ValueError on a bad combination.  Returns
    get_samples' pag = (scale, layers_first, layers_late) or None.  --pag_layers names the blocks of the only model, or of the late model
    of a pair; --pag_layers_first those of the first model of a pair."""
    if args.pag_scale is None:
        if args.pag_layers is not None or args.pag_layers_first is not None:
            raise ValueError("--pag_layers / --pag_layers_first need --pag_scale")
        return None
    if not math.isfinite(args.pag_scale):
        raise ValueError("--pag_scale must be finite")
    for name in ("cfg_scale", "autoguidance_scale", "known_image", "init_image", "clip_x0", "dynamic_threshold"):
        if getattr(args, name, None) is not None:
            raise ValueError(f"--pag_scale and --{name} are exclusive")
    depth = ModelParams.from_dict(config).depth
    if config_late is None:
        if args.pag_layers_first is not None:
            raise ValueError("--pag_layers_first is for the first model of a pair (--checkpoint_path_late); use --pag_layers")
        return args.pag_scale, pag_layers(args.pag_layers, depth, "--pag_layers"), []
    depth_late = ModelParams.from_dict(config_late).depth
    return (args.pag_scale, pag_layers(args.pag_layers_first, depth, "--pag_layers_first"),
            pag_layers(args.pag_layers, depth_late, "--pag_layers"))


def _load_image_file(path, what, mp, latent, pixels=False):
    """--init_image / --known_image / --known_mask: a .npy in the model's own space, or (pixel-space RGB models, and latent models under
    --encode_images: pixels) a .png mapped through 2 v - 1 (the mask: its first channel, unmapped) -> float32 [N, C, S, S]"""
    path = Path(path)
    mask = what == "--known_mask"
    if path.suffix.lower() == ".npy":
        a = np.asarray(np.load(path), np.float32)
    elif path.suffix.lower() == ".png":
        if latent and not pixels:
            raise ValueError(f"{what} {path.name}: a latent model takes .npy latents only, or pixel-space files with --encode_images")
        if mp.in_chans != 3 and not pixels:
            raise ValueError(f"{what} {path.name}: .png needs an in_chans = 3 config, this one has in_chans = {mp.in_chans}")
        from matplotlib import pyplot as plt
        a = np.asarray(plt.imread(path), np.float32)
        a = a[..., None] if a.ndim == 2 else a
        a = a[..., :1] if mask else 2.0 * (a[..., :3] if a.shape[-1] >= 3 else np.repeat(a[..., :1], 3, -1)) - 1.0
        a = np.ascontiguousarray(a.transpose(2, 0, 1))[None]
    else:
        raise ValueError(f"{what} {path.name}: .npy or .png")
    return a


def validate_region(args, config):
    """The image-to-image and inpainting options against the config, before any GPU work: ValueError on a bad combination.  Returns
    get_samples' init_image / strength / known_image / known_mask arguments, the files loaded.  With --encode_images the files are in
    pixel space ([.., 3, 8 S, 8 S] images in [-1, 1], a [.., 1, 8 S, 8 S] mask) and main() passes the result through encode_region once
    the autoencoder is loaded."""
    mp = ModelParams.from_dict(config)
    pixels = bool(getattr(args, "encode_images", False))
    if pixels:
        if "autoencoder" not in config:
            raise ValueError("--encode_images needs a latent model (a config with an autoencoder block); a pixel-space model takes its images as they are")
        if args.init_image is None and args.known_image is None:
            raise ValueError("--encode_images needs --init_image or --known_image")
        if mp.in_chans != 4 or mp.img_size % 8 or mp.img_size > 32:
            raise ValueError(f"--encode_images: the KL-VAE encoder gives 4-channel latents of a size that is a multiple of 8, at most 32; "
                             f"this config has in_chans = {mp.in_chans}, img_size = {mp.img_size}")
    elif getattr(args, "encode_mean", False):
        raise ValueError("--encode_mean goes with --encode_images")
    size = 8 * mp.img_size if pixels else mp.img_size
    if (args.known_image is None) != (args.known_mask is None):
        raise ValueError("--known_image and --known_mask go together")
    if (args.init_image is None) != (args.strength is None):
        raise ValueError("--init_image and --strength go together")
    if args.strength is not None and not 0 < args.strength <= 1:
        raise ValueError(f"--strength {args.strength} outside (0, 1]")
    out = dict(init_image=None, strength=args.strength, known_image=None, known_mask=None)
    for key, chans in (("init_image", 3 if pixels else mp.in_chans), ("known_image", 3 if pixels else mp.in_chans), ("known_mask", 1)):
        path = getattr(args, key)
        if path is None:
            continue
        a = _load_image_file(path, "--" + key, mp, "autoencoder" in config, pixels)
        if a.ndim != 4 or a.shape[0] not in (1, args.batch_size) or a.shape[1:] != (chans, size, size):
            raise ValueError(f"--{key}: shape {list(a.shape)} does not match [1 or {args.batch_size}, {chans}, {size}, {size}]")
        if not np.isfinite(a).all() or (key == "known_mask" and ((a < 0) | (a > 1)).any()):
            raise ValueError(f"--{key}: " + ("values outside [0, 1]" if key == "known_mask" else "non-finite values"))
        out[key] = a
    return out


def reduce_mask_8x8(mask):
    """A pixel-space mask [N, 1, 8 S, 8 S] at latent resolution [N, 1, S, S]: the minimum over every 8 x 8 block.  A latent pixel counts
    as known only if every pixel under it is, so the generated region never shrinks, and a binary mask stays binary."""
    m = np.asarray(mask, np.float32)
    n, c, h, w = m.shape
    return np.ascontiguousarray(m.reshape(n, c, h // 8, 8, w // 8, 8).min(axis=(3, 5)))


def encode_region(region_kwargs, autoencoder, seed, mean=False):
    """--encode_images: validate_region's pixel-space files -> what get_samples takes.  Each image goes through autoencoder.encode with a
    generator of its own seeded with `seed` (the loop's noise streams are what they are without the flag), or its mode (mean); the mask
    through reduce_mask_8x8."""
    out = dict(region_kwargs)
    for key in ("init_image", "known_image"):
        if out[key] is not None:
            z = autoencoder.encode(torch.from_numpy(out[key]), generator=torch.Generator().manual_seed(int(seed)), sample=not mean)
            out[key] = z.cpu().numpy()
    if out["known_mask"] is not None:
        out["known_mask"] = reduce_mask_8x8(out["known_mask"])
    return out


SOLVERS = {"ode": "dpmsolver++", "sde": "sde-dpmsolver++"}


def validate_solver(args):
    """The DPM-Solver++ options, before any GPU work: ValueError on a bad combination."""
    if args.dpm_solver is None:
        return
    if args.use_ddim:
        raise ValueError("--dpm_solver and --use_ddim are exclusive")
    if args.parametrization == "predict_previous":
        raise ValueError("--dpm_solver needs --parametrization predict_noise or predict_original, not predict_previous")
    if not 1 <= args.dpm_solver_steps <= 999:
        raise ValueError(f"--dpm_solver_steps {args.dpm_solver_steps} outside [1, 999]")


def validate_threshold(args, config):
    """The x0 thresholding options against the config, before any GPU work: ValueError on a bad combination.  Returns get_samples'
    threshold argument (None: off)."""
    clip, dyn, smax = args.clip_x0, args.dynamic_threshold, args.threshold_max
    if clip is None and dyn is None:
        if smax is not None:
            raise ValueError("--threshold_max goes with --dynamic_threshold")
        return None
    if clip is not None and dyn is not None:
        raise ValueError("--clip_x0 and --dynamic_threshold are exclusive")
    if "autoencoder" in config:
        raise ValueError("--clip_x0 / --dynamic_threshold are for pixel-space models: with an autoencoder block x0 is a latent, not an image in [-1, 1]")
    if args.parametrization == "predict_previous":
        raise ValueError("--clip_x0 / --dynamic_threshold need --parametrization predict_noise or predict_original: predict_previous has no x0")
    if args.noise == "torch_cpu":
        raise ValueError("--clip_x0 / --dynamic_threshold run in the device-resident loops: --noise device")
    if clip is not None:
        if smax is not None:
            raise ValueError("--threshold_max goes with --dynamic_threshold")
        if not (clip > 0 and math.isfinite(clip)):
            raise ValueError(f"--clip_x0 {clip} must be positive and finite")
        return X0Threshold("static", range=float(clip))
    if not 0 < dyn <= 1:
        raise ValueError(f"--dynamic_threshold {dyn} outside (0, 1]")
    smax = float("inf") if smax is None else float(smax)
    if not smax >= 1:
        raise ValueError(f"--threshold_max {smax} must be at least 1")
    return X0Threshold("dynamic", quantile=float(dyn), s_max=smax)


def validate_resample(args):
    """The resampling options (--resample_jump / --resample_count, --restart), before any GPU work: ValueError on a bad combination.
    Returns get_samples' resample_jump / resample_count / restart arguments.  What depends on the grid (an interval that holds fewer than
    two of its levels, overlaps) is step_plan's to reject, still before any GPU work."""
    j, r, restart = args.resample_jump, args.resample_count, args.restart
    if (j is None) != (r is None):
        raise ValueError("--resample_jump and --resample_count go together")
    if j is None and not restart:
        return dict(resample_jump=None, resample_count=None, restart=None)
    if j is not None and restart:
        raise ValueError("--resample_jump / --resample_count (RePaint) and --restart are exclusive")
    if j is not None and j < 1:
        raise ValueError(f"--resample_jump {j} must be at least 1")
    if r is not None and r < 1:
        raise ValueError(f"--resample_count {r} must be at least 1")
    for name in ("dpm_solver", "clip_x0", "dynamic_threshold", "pag_scale"):
        if getattr(args, name, None) is not None:
            raise ValueError(f"--resample_jump / --restart and --{name} are exclusive")
    out = []
    for t_min, t_max, k in restart or ():
        if k != int(k) or k < 1:
            raise ValueError(f"--restart {t_min:g} {t_max:g} {k:g}: K must be a whole number, at least 1")
        if not 0 <= t_min < t_max <= 999:
            raise ValueError(f"--restart {t_min:g} {t_max:g} {k:g}: need 0 <= T_MIN < T_MAX <= 999")
        out.append((float(t_min), float(t_max), int(k)))
    kw = dict(resample_jump=j, resample_count=r, restart=out or None)
    step_plan(args.parametrization, use_ddim=args.use_ddim, ddim_steps=args.ddim_steps, ddim_eta=args.ddim_eta, strength=args.strength, **kw)
    return kw


def validate_cache(args, config, config_late=None):
    """The block-caching options (--cache_blocks, --cache_interval, --cache_order), before any GPU work: ValueError on a bad combination.
    Returns get_samples' cache argument, (K, N, order) or None."""
    if args.cache_blocks is None:
        if args.cache_interval is not None or args.cache_order is not None:
            raise ValueError("--cache_interval / --cache_order need --cache_blocks")
        return None
    for name in ("dpm_solver", "clip_x0", "dynamic_threshold", "resample_jump", "restart", "pag_scale", "autoguidance_scale"):
        if getattr(args, name, None) is not None:
            raise ValueError(f"--cache_blocks and --{name} are exclusive")
    depths = [ModelParams.from_dict(c).depth for c in (config, config_late) if c is not None]
    return cache_settings(args.cache_blocks, 3 if args.cache_interval is None else args.cache_interval,
                          0 if args.cache_order is None else args.cache_order, depths=depths)


def solver_kwargs(args):
    """get_samples' solver arguments from the command line"""
    return dict(solver=SOLVERS[args.dpm_solver] if args.dpm_solver is not None else None, solver_steps=args.dpm_solver_steps,
                solver_order=args.dpm_solver_order)


def image_seed_list(args, batch_size: int, first_image=None):
    """--image_seeds: image i of the run (i counted from --first_image, or from first_image) gets seed --seed + i; None without the flag"""
    if not getattr(args, "image_seeds", False):
        return None
    first = int(args.first_image if first_image is None else first_image)       # (validate_image_seeds: not negative)
    return [int(args.seed) + first + i for i in range(int(batch_size))]


def validate_image_seeds(args):
    """--image_seeds / --first_image against the noise mode, before any GPU work"""
    if getattr(args, "first_image", 0) < 0:
        raise ValueError("--first_image must not be negative")
    if not getattr(args, "image_seeds", False):
        if getattr(args, "first_image", 0):
            raise ValueError("--first_image needs --image_seeds")
        return
    if args.noise != "device":
        raise ValueError("--image_seeds needs --noise device: the torch CPU stream is sequential in the batch")


def draw_labels_per_image(seeds, num_classes: int):
    """--class_id's draw (quirk Q4: randint(1, 1001) whatever the id) per image: label i is a function of seeds[i] alone"""
    return draw_labels(len(seeds), num_classes, seeds)


def labels_from_args(args, batch_size: int, num_classes: int, image_seeds=None):
    """y of a run: --class_label K for every image, --class_id's reference draw (quirk Q4; with image_seeds: per image), or None."""
    if getattr(args, "class_label", None) is not None:                      # (eesampler has --class_id only)
        return torch.full((batch_size,), int(args.class_label), dtype=torch.int64)
    if args.class_id is not None:
        return draw_labels(batch_size, num_classes, image_seeds)
    return None


def dump_samples(samples, output_folder: Path, timestep=1000):
    """reference sampler.py:158-184: per-image PNG + grid, values clipped to [0, 1]."""
    from matplotlib import pyplot as plt
    n = len(samples)
    grid = math.ceil(math.sqrt(n))
    h, w = samples[0].shape[:2]
    grid_img = np.zeros((grid * h, grid * w, 3))
    for i, s in enumerate(samples):
        s = np.clip(s, 0, 1)
        name = f"{i}_{timestep}.png" if timestep != 1000 else f"{i}.png"
        plt.imsave(output_folder / name, s)
        r, c = divmod(i, grid)
        grid_img[r * h:(r + 1) * h, c * w:(c + 1) * w, :] = s[..., :3]
    plt.imsave(output_folder / "grid_image.png", grid_img)


def dump_statistics(elapsed_time, output_folder: Path, batch_size=None):
    with open(output_folder / "statistics.txt", "w") as f:
        f.write(f"Elapsed time: {elapsed_time} s\n")                          # reference sampler.py:187-189
        if batch_size:
            f.write(f"Images per second: {batch_size / elapsed_time}\n")


def add_image_seed_args(p):
    """the per-image seed flags the three command lines share (sampler, dist, eesampler)"""
    p.add_argument("--image_seeds", action="store_true",
                   help="(engine option) image i of the run gets its own seed, --seed + --first_image + i, and depends on nothing else: the "
                        "same pictures at any --batch_size and on any number of GPUs.  Needs --noise device")
    p.add_argument("--first_image", type=int, default=0, metavar="N",
                   help="(engine option) with --image_seeds: the run's first image is image N (regenerate image i alone with "
                        "--first_image i --batch_size 1)")


def get_args(argv=None):
    p = ArgumentParser()
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--checkpoint_path", type=str, required=True, help="Path to checkpoint of the model")
    p.add_argument("--autoencoder_checkpoint_path", type=str, default=None,
                   help="(engine option) overrides config['autoencoder']['autoencoder_checkpoint_path']")
    p.add_argument("--checkpoint_path_late", type=str, default=None,
                   help="Path to checkpoint of the model to be used in the latest steps")
    p.add_argument("--batch_size", type=int, required=True)
    p.add_argument("--parametrization", type=str, required=True,
                   choices=["predict_noise", "predict_original", "predict_previous"])
    p.add_argument("--output_folder", type=str, required=True)
    p.add_argument("--config_path", type=str, required=True, help="Path to yaml config file")
    p.add_argument("--config_path_late", type=str, default=None,
                   help="Path to yaml config file of the model to be used in the latest steps")
    p.add_argument("--t_switch", type=int, default=np.inf,
                   help="Sampling timestep where the model should be replaced by the late model")
    p.add_argument("--class_id", type=int, default=None, help="Number up to 1000 that corresponds to a class")
    p.add_argument("--use_ddim", action="store_true")
    p.add_argument("--ddim_steps", type=int, default=50)
    p.add_argument("--ddim_eta", type=float, default=0.0)
    p.add_argument("--timesteps_save", type=int, nargs="+", default=[])
    # engine options (not in the reference)
    p.add_argument("--precision", choices=["bf16", "fp32"], default="bf16")
    p.add_argument("--noise", choices=["torch_cpu", "device"], default="device")
    p.add_argument("--no_graph", action="store_true", help="launch kernels eagerly instead of hipGraph replay")
    p.add_argument("--no_png", action="store_true", help="write samples.npy instead of PNG files")
    p.add_argument("--class_label", type=int, default=None,
                   help="(engine option) every image gets this class label (what --class_id's help promises; --class_id keeps the "
                        "reference's random draw)")
    p.add_argument("--cfg_scale", type=float, default=None,
                   help="(engine option) classifier-free guidance eps = eps_c + S (eps_c - eps_u); any value, 0 included, selects the "
                        "guided loops (default: unguided).  Needs a class-conditional config with a null-class row and --class_label or "
                        "--class_id; an image whose drawn --class_id label equals the null label is sampled unguided")
    p.add_argument("--cfg_null_label", type=int, default=1000,
                   help="(engine option) label of the unconditional rows (default 1000: U-ViT's null class)")
    p.add_argument("--autoguidance_scale", type=float, default=None,
                   help="(engine option) autoguidance eps = eps_m + S (eps_m - eps_guide): every step of a model other than the guide runs "
                        "the guide on the same rows; any value, 0 included, selects it (default: off).  Without an explicit guide the first "
                        "(shallow) model guides the late one and --checkpoint_path_late is required.  Exclusive with --cfg_scale")
    p.add_argument("--pag_scale", type=float, default=None,
                   help="(engine option) perturbed-attention guidance eps = eps + S (eps - eps_perturbed), eps_perturbed the same model with "
                        "identity self-attention in the blocks of --pag_layers; any value, 0 included, selects the path (2 B backbone rows). "
                        "Needs no labels and no second model.  Exclusive with --cfg_scale, --autoguidance_scale, --known_image, --init_image, "
                        "--clip_x0 and --dynamic_threshold")
    p.add_argument("--pag_layers", type=str, nargs="+", default=None, metavar="mid|I",
                   help="(engine option) blocks with identity attention, by index in forward order (in_blocks, mid_block, out_blocks), of the "
                        "only model or of the late model of a pair; default: mid = block depth // 2")
    p.add_argument("--pag_layers_first", type=str, nargs="+", default=None, metavar="mid|I",
                   help="(engine option) the same for the first model of a pair; default: mid")
    p.add_argument("--guide_config_path", type=str, default=None,
                   help="(engine option) yaml config of an explicit guide model (same img_size, patch_size, in_chans)")
    p.add_argument("--guide_checkpoint_path", type=str, default=None, help="(engine option) checkpoint of the explicit guide model")
    p.add_argument("--dpm_solver", choices=sorted(SOLVERS), default=None,
                   help="(engine option) DPM-Solver++ multistep sampling: ode = DPM-Solver++(2M), sde = SDE-DPM-Solver++(2M) "
                        "(default: the reference's loops).  Exclusive with --use_ddim; predict_noise / predict_original models")
    p.add_argument("--dpm_solver_steps", type=int, default=20, help="(engine option) DPM-Solver++ model evaluations, 1 .. 999")
    p.add_argument("--dpm_solver_order", type=int, choices=[1, 2], default=2, help="(engine option) DPM-Solver++ order")
    p.add_argument("--init_image", type=str, default=None,
                   help="(engine option) image-to-image: start from this image (.npy in the model's space [1 or B, C, S, S], or .png for "
                        "RGB pixel models) noised to t = round(999 * --strength)")
    p.add_argument("--strength", type=float, default=None, help="(engine option) in (0, 1]: how far --init_image is noised; 1 = pure noise")
    p.add_argument("--known_image", type=str, default=None,
                   help="(engine option) inpainting: the image whose --known_mask region stays fixed (.npy / .png as --init_image)")
    p.add_argument("--known_mask", type=str, default=None,
                   help="(engine option) inpainting mask in [0, 1], 1 = keep (.npy [1 or B, 1, S, S], or the first channel of a .png)")
    p.add_argument("--encode_images", action="store_true",
                   help="(engine option) latent models: --init_image / --known_image / --known_mask are in pixel space (.png or .npy "
                        "[1 or B, 3, 8S, 8S] in [-1, 1]; mask [1 or B, 1, 8S, 8S]); the images go through the KL-VAE encoder, the mask "
                        "through an 8x8 minimum")
    p.add_argument("--encode_mean", action="store_true",
                   help="(engine option) with --encode_images: the posterior's mode 0.18215 mean instead of a sample")
    p.add_argument("--clip_x0", type=float, nargs="?", const=1.0, default=None, metavar="R",
                   help="(engine option) clip every step's predicted image x0 to [-R, R] (default R = 1) before it drives the update")
    p.add_argument("--dynamic_threshold", type=float, default=None, metavar="Q",
                   help="(engine option) dynamic thresholding (Imagen): per image, s = the Q-quantile of |x0| (at least 1), x0 clipped to "
                        "[-s, s] and divided by s.  Exclusive with --clip_x0; pixel-space predict_noise / predict_original models, --noise device")
    p.add_argument("--threshold_max", type=float, default=None, metavar="S", help="(engine option) with --dynamic_threshold: s is at most S (>= 1)")
    p.add_argument("--resample_jump", type=int, default=None, metavar="J",
                   help="(engine option) RePaint's resampling: every J grid steps x is noised back up J steps (no model evaluation) and "
                        "brought down again; with --resample_count.  DDPM and DDIM loops, with or without --known_image")
    p.add_argument("--resample_count", type=int, default=None, metavar="R",
                   help="(engine option) with --resample_jump: each stretch of J steps is run R times in all (1: no jumps)")
    p.add_argument("--restart", type=float, nargs=3, action="append", default=None, metavar=("T_MIN", "T_MAX", "K"),
                   help="(engine option, repeatable) Restart sampling: having come down to the timestep T_MIN the loop goes back up to T_MAX "
                        "with fresh noise and comes down again, K times; intervals snap to the grid and must not overlap.  Exclusive with "
                        "--resample_jump")
    p.add_argument("--cache_blocks", type=int, default=None, metavar="K",
                   help="(engine option) block caching (DeepCache): only every N-th step of a model runs its deep blocks K .. depth - 1 - K; "
                        "the steps between reuse their stored output.  1 <= K <= depth // 2 of every model.  DDPM and DDIM loops")
    p.add_argument("--cache_interval", type=int, default=None, metavar="N",
                   help="(engine option) with --cache_blocks: a full step every N steps of a model (default 3; 1: every step)")
    p.add_argument("--cache_order", type=int, choices=[0, 1], default=None,
                   help="(engine option) with --cache_blocks: 0 (default) reuses the stored output, 1 extrapolates the last two linearly in t")
    add_image_seed_args(p)
    return p.parse_args(argv)


def load_checkpoint(path):
    """reference sampler.py:289-291: a bare state_dict or {"model_state_dict": ...}."""
    sd = torch.load(path, map_location="cpu")
    return sd["model_state_dict"] if "model_state_dict" in sd else sd


def build_model(config, checkpoint_path, precision, max_batch):
    mp = ModelParams.from_dict(config)
    m = UViT(**mp.as_dict(), precision=precision, max_batch=max_batch)
    m.load_state_dict(load_checkpoint(checkpoint_path))
    return m.eval().to(get_device()), mp


def load_autoencoder(args, config, device):
    """The KL-VAE a latent model's config names (reference sampler.py:320-325; --autoencoder_checkpoint_path overrides), or None"""
    if "autoencoder" in config:
        path = args.autoencoder_checkpoint_path or config["autoencoder"]["autoencoder_checkpoint_path"]
        return get_autoencoder(path, precision=args.precision).to(device)


RunSetup = namedtuple("RunSetup", "mp kwargs")


def setup_run(args):
    """Everything between get_args and get_samples, for sampler.main and dist.main alike: every validate_* (all before the first model is
    built), the configs, the models on backbone_rows rows (an explicit guide included), the autoencoder, --encode_images.  -> RunSetup(mp:
    the first model's ModelParams; kwargs: get_samples' arguments but seed, image_seeds, y, timesteps_save and return_device_tensor)"""
    validate_solver(args)
    validate_image_seeds(args)
    config = load_config(args.config_path)
    config_late = load_config(args.config_path_late) if args.checkpoint_path_late else None
    validate_guidance(args, ModelParams.from_dict(config).num_classes, config_late and ModelParams.from_dict(config_late).num_classes)
    config_guide = load_config(args.guide_config_path) if args.guide_config_path else None
    validate_autoguidance(args, config, config_late, config_guide)
    config_last = config_late if config_late is not None else config        # (the model that finishes the images)
    region_kwargs = validate_region(args, config_last)
    threshold = validate_threshold(args, config_last)
    pag = validate_pag(args, config, config_late)
    resample = validate_resample(args)
    cache = validate_cache(args, config, config_late)
    rows = backbone_rows(args.batch_size, args.cfg_scale, pag)
    model, mp = build_model(config, args.checkpoint_path, args.precision, rows)
    late = build_model(config_late, args.checkpoint_path_late, args.precision, rows)[0] if config_late is not None else None
    guide = build_model(config_guide, args.guide_checkpoint_path, args.precision, rows)[0] if config_guide is not None else None
    autoencoder = load_autoencoder(args, config_last, model.device)
    if args.encode_images:
        print("Encode the images...")
        region_kwargs = encode_region(region_kwargs, autoencoder, args.seed, mean=args.encode_mean)
    post = {name: fn for fn, name in _PARAMETRIZATIONS.items()}[args.parametrization]
    return RunSetup(mp, dict(
        model=model, batch_size=args.batch_size, postprocessing=post, num_channels=mp.in_chans, sample_height=mp.img_size,
        sample_width=mp.img_size, use_ddim=args.use_ddim, ddim_steps=args.ddim_steps, ddim_eta=args.ddim_eta, autoencoder=autoencoder,
        late_model=late, t_switch=args.t_switch, noise=args.noise, use_graph=not args.no_graph, cfg_scale=args.cfg_scale,
        cfg_null_label=args.cfg_null_label, **solver_kwargs(args), autoguidance_scale=args.autoguidance_scale, guide_model=guide,
        threshold=threshold, pag=pag, cache=cache, **resample, **region_kwargs))


def main(argv=None):
    args = get_args(argv)
    out = Path(args.output_folder)
    out.mkdir(parents=True, exist_ok=True)
    setup = setup_run(args)
    seed_everything(args.seed)
    image_seeds = image_seed_list(args, args.batch_size)
    y = labels_from_args(args, args.batch_size, setup.mp.num_classes, image_seeds)
    tic = time.time()
    samples, inter = get_samples(**setup.kwargs, seed=args.seed, image_seeds=image_seeds, y=y, timesteps_save=args.timesteps_save)
    tac = time.time()
    dump_statistics(tac - tic, out, args.batch_size)
    if args.no_png:
        np.save(out / "samples.npy", samples)
    else:
        dump_samples(samples, out)
        for ts, smp in zip(args.timesteps_save, inter):
            dump_samples(smp, out, ts)
    print(f"Elapsed time: {tac - tic} s  ({args.batch_size / (tac - tic):.3f} images/s)")


if __name__ == "__main__":
    main()
