"""ctypes binding of libduodiff.so (include/duodiff.h).  No CPU fallback: a missing
library is an ImportError-class failure raised at first use, loudly."""
import ctypes as C
import os
from pathlib import Path

LIB_PATH = Path(os.environ.get("DUODIFF_LIB") or Path(__file__).resolve().parent / "libduodiff.so")

DD_OK = 0
DD_ERR_INVALID, DD_ERR_NOT_FOUND, DD_ERR_STATE, DD_ERR_HIP, DD_ERR_NOMEM, DD_ERR_UNSUPPORTED = -1, -2, -3, -4, -5, -6
DD_PREC_BF16, DD_PREC_FP32 = 0, 1
DD_VAR_BETA_TILDE, DD_VAR_BETA = 0, 1
DD_NOISE_NONE, DD_NOISE_BUFFER, DD_NOISE_PHILOX = 0, 1, 2
DD_X0_STATIC, DD_X0_DYNAMIC = 0, 1
DD_EE_MLP_PER_LAYER, DD_EE_MLP_PER_TIMESTEP, DD_EE_MLP_PER_LAYER_PER_TIMESTEP, DD_EE_ATTENTION_PROBE = 0, 1, 2, 3
ABI_VERSION = 6
DD_DEV_NO_FUSED_MLP, DD_DEV_NO_FUSED_PROJ, DD_DEV_NO_FUSED_HEAD, DD_DEV_GENERIC_EMBED, DD_DEV_MLP_EXTRAS_ONLY = 1, 2, 4, 8, 16
DD_DEV_NO_FUSED_SKIP, DD_DEV_NO_FUSED_QKV, DD_DEV_NO_FUSED_QA = 32, 64, 128
DD_PROF_DOMINANT, DD_PROF_BLOCK_TAIL, DD_PROF_FC1, DD_PROF_ROWLIN, DD_PROF_QKV_ATTENTION, DD_PROF_SPLITK = 0, 1, 2, 3, 4, 5
DD_DEV_NO_CHAINS, DD_DEV_FORCE_CHAINS, DD_DEV_NO_ROWLIN, DD_DEV_NO_ROWLIN_PROJ, DD_DEV_NO_EMBED_LN, DD_DEV_NO_SPLITK, DD_DEV_NO_ROWLIN_SKIP = 256, 512, 1024, 2048, 4096, 8192, 16384
DD_DEV_NO_SPLIT_HEADS = 32768
DD_DEV_NO_FRAG_AO, DD_DEV_NO_FRAG_SKIP, DD_DEV_NO_FRAG_X = 65536, 131072, 262144


class dd_config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "img_size", "patch_size", "in_chans", "embed_dim", "depth", "num_heads", "mlp_ratio",
        "num_classes", "normalize_timesteps", "max_batch", "qkv_bias", "mlp_time_embed")]


class dd_sample_args(C.Structure):
    _fields_ = [("first", C.c_void_p), ("late", C.c_void_p), ("t_switch", C.c_int32),
                ("t_start", C.c_int32), ("t_end", C.c_int32), ("variance", C.c_int32),
                ("noise_mode", C.c_int32), ("use_graph", C.c_int32), ("seed", C.c_uint64),
                ("y_dev", C.c_void_p), ("x_dev", C.c_void_p), ("B", C.c_int32), ("reserved", C.c_int32)]


class dd_affine_sample_args(C.Structure):
    _fields_ = [("first", C.c_void_p), ("late", C.c_void_p), ("n_steps", C.c_int32), ("switch_after", C.c_int32),
                ("t", C.POINTER(C.c_float)), ("a", C.POINTER(C.c_float)), ("b", C.POINTER(C.c_float)),
                ("c", C.POINTER(C.c_float)), ("noise", C.POINTER(C.c_int32)), ("noise_mode", C.c_int32),
                ("use_graph", C.c_int32), ("seed", C.c_uint64), ("y_dev", C.c_void_p), ("x_dev", C.c_void_p),
                ("B", C.c_int32), ("counter_base", C.c_int32)]


class dd_multistep_sample_args(C.Structure):
    """dd_affine_sample_args' fields, then the history half of the rows and the history register (include/duodiff.h)"""
    _fields_ = dd_affine_sample_args._fields_ + [
        ("d", C.POINTER(C.c_float)), ("p", C.POINTER(C.c_float)), ("q", C.POINTER(C.c_float)), ("hist", C.POINTER(C.c_int32)),
        ("h_dev", C.c_void_p)]


class dd_guidance(C.Structure):
    """classifier-free guidance: eps = eps_c + scale * (eps_c - eps_u), the unconditional rows labelled null_label"""
    _fields_ = [("scale", C.c_float), ("null_label", C.c_int32)]


class dd_autoguidance(C.Structure):
    """autoguidance: eps = eps_main + scale * (eps_main - eps_guide), guide = the weaker dd_model of the same image geometry"""
    _fields_ = [("guide", C.c_void_p), ("scale", C.c_float)]


class dd_pag(C.Structure):
    """perturbed-attention guidance: eps = eps + scale * (eps - eps_perturbed), identity attention in the blocks of the model's mask"""
    _fields_ = [("scale", C.c_float), ("layers_first", C.c_uint32), ("layers_late", C.c_uint32)]


class dd_known_region(C.Structure):
    """a known region: x' is finished as m * (ka x0 + kb z2) + (1 - m) x' from the known image x0, the mask m and per-step rows ka, kb"""
    _fields_ = [("x0_dev", C.c_void_p), ("mask_dev", C.c_void_p), ("ka", C.POINTER(C.c_float)), ("kb", C.POINTER(C.c_float))]


class dd_walk(C.Structure):
    """a walk's per-row program beside the step table: jump[k] != 0: row k is a resampling jump; late[k] (or NULL): step row k runs the late model"""
    _fields_ = [("jump", C.POINTER(C.c_int32)), ("late", C.POINTER(C.c_int32))]


class dd_block_cache(C.Structure):
    """block caching beside the step table: K = blocks, the order, and per step the op (0 refresh, 1 reuse, 2 reuse with extrapolation) and its weight"""
    _fields_ = [("blocks", C.c_int32), ("order", C.c_int32), ("op", C.POINTER(C.c_int32)), ("w", C.POINTER(C.c_float))]


class dd_x0_threshold(C.Structure):
    """x0 thresholding of the multistep loop: static (clamp to +-range) or dynamic (the image's own quantile scale, at most s_max)"""
    _fields_ = [("mode", C.c_int32), ("quantile", C.c_float), ("range", C.c_float), ("s_max", C.c_float)]


class dd_ee_sample_args(C.Structure):
    _fields_ = [("model", C.c_void_p), ("threshold", C.c_float), ("t_start", C.c_int32), ("t_end", C.c_int32),
                ("noise_mode", C.c_int32), ("use_graph", C.c_int32), ("B", C.c_int32), ("seed", C.c_uint64),
                ("y_dev", C.c_void_p), ("x_dev", C.c_void_p), ("err_dev", C.c_void_p), ("idx_dev", C.c_void_p)]


class dd_ee_real(C.Structure):
    """dd_sample_early_exit_real: layers l with l % compact_every == 0 compact the batch"""
    _fields_ = [("compact_every", C.c_int32), ("reserved", C.c_int32)]


class dd_scan_args(C.Structure):
    """dd_scan_error (include/duodiff.h): the images, the scan's rows and where the per-image errors go"""
    _fields_ = [("model", C.c_void_p), ("x0_dev", C.c_void_p), ("y_dev", C.c_void_p), ("B", C.c_int32), ("n_steps", C.c_int32)] + \
               [(n, C.POINTER(C.c_float)) for n in ("t", "ka", "kb", "tz", "t0", "tx")] + \
               [("seed", C.c_uint64), ("counter_base", C.c_int32), ("noise_mode", C.c_int32), ("use_graph", C.c_int32),
                ("reserved", C.c_int32), ("err_dev", C.c_void_p)]
    x_dev = property(lambda self: self.x0_dev, lambda self, v: setattr(self, "x0_dev", v))     # (the name engine._run_loop fills the image tensor in by)


class dd_dev_scan_args(C.Structure):
    """the operands of dd_dev_scan_diffuse / dd_dev_scan_error (include/duodiff_dev.h), field for field"""
    _fields_ = ([(n, C.c_int32) for n in ("B", "C", "S", "b0", "B_all", "k")] +
                [(n, C.c_float) for n in ("t_model", "ka", "kb", "tz", "t0", "tx")] +
                [("ctr", C.c_int32), ("next_t_model", C.c_float), ("seed", C.c_uint64), ("advance", C.c_int32), ("t_out", C.c_int32),
                 ("t_final_out", C.c_int32), ("t_model_out", C.c_float), ("iters", C.c_int32), ("ms_out", C.c_float)])


class dd_scan_exits_args(C.Structure):
    """dd_scan_error_early_exit (include/duodiff.h): dd_scan_args with the three result tables in err_dev's place"""
    _fields_ = dd_scan_args._fields_[:-1] + [("mse_dev", C.c_void_p), ("target_dev", C.c_void_p), ("pred_dev", C.c_void_p)]
    x_dev = property(lambda self: self.x0_dev, lambda self, v: setattr(self, "x0_dev", v))


class dd_dev_scan_exits_args(C.Structure):
    """the operands of dd_dev_scan_exits_error (include/duodiff_dev.h), field for field"""
    _fields_ = ([(n, C.c_int32) for n in ("B", "C", "S", "exits", "b0", "B_all", "k", "t", "next")] +
                [(n, C.c_float) for n in ("t_model", "ka", "kb", "tz", "t0", "tx")] +
                [("ctr", C.c_int32), ("next_t_model", C.c_float), ("seed", C.c_uint64), ("advance", C.c_int32), ("t_out", C.c_int32),
                 ("t_final_out", C.c_int32), ("t_model_out", C.c_float), ("iters", C.c_int32), ("ms_out", C.c_float)])


class dd_dev_final_args(C.Structure):
    """the operands of dd_dev_final (include/duodiff_dev.h), field for field"""
    _fields_ = ([(n, C.c_int32) for n in ("B", "C", "S", "P", "L", "extras", "b0", "images")] +
                [(n, C.c_void_p) for n in ("dec", "wconv", "bconv", "dec2", "wconv2", "bconv2")] +
                [(n, C.c_int32) for n in ("L2", "extras2", "pair_B", "layer_B")] +
                [("w_stride", C.c_int64), ("b_stride", C.c_int64), ("guide_scale", C.c_float)] +
                [(n, C.c_int32) for n in ("write_eps", "write_x", "x_alias")] +
                [(n, C.c_void_p) for n in ("eps_out", "x_out", "x_in", "z")] +
                [(n, C.c_int32) for n in ("t", "advance", "noise_mode", "variance")] +
                [("seed", C.c_uint64), ("table", C.c_int32)] +
                [(n, C.c_float) for n in ("c1", "c2", "sigma_tilde", "sigma_beta", "row_t_model", "row_a", "row_b", "row_c")] +
                [("row_noise", C.c_int32), ("row_ctr", C.c_int32), ("next_t_model", C.c_float), ("hist_row", C.c_int32)] +
                [(n, C.c_float) for n in ("hist_d", "hist_p", "hist_q")] +
                [("hist", C.c_int32), ("h", C.c_void_p), ("known", C.c_int32), ("known_ka", C.c_float), ("known_kb", C.c_float),
                 ("kx0", C.c_void_p), ("kmask", C.c_void_p), ("t_out", C.c_int32), ("t_final_out", C.c_int32), ("t_model_out", C.c_float),
                 ("seed_out", C.c_uint64)])


# every symbol include/duodiff.h (and include/duodiff_dev.h: dd_dev_*) declares: name -> (restype, argtypes)
SIGNATURES = {
    "dd_abi_version": (C.c_int, []),
    "dd_build_id": (C.c_char_p, []),
    "dd_ctx_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "dd_ctx_destroy": (None, [C.c_void_p]),
    "dd_last_error": (C.c_char_p, [C.c_void_p]),
    "dd_sync": (C.c_int, [C.c_void_p, C.c_void_p]),
    "dd_schedule_table": (C.c_int, [C.c_int, C.POINTER(C.c_float)]),
    "dd_schedule_build": (C.c_int, [C.c_float, C.c_float, C.c_int] + [C.POINTER(C.c_float)] * 5),
    "dd_model_create": (C.c_int, [C.c_void_p, C.POINTER(dd_config), C.POINTER(C.c_void_p)]),
    "dd_model_set_param": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int]),
    "dd_model_finalize": (C.c_int, [C.c_void_p, C.c_int]),
    "dd_model_num_params": (C.c_int64, [C.c_void_p]),
    "dd_model_destroy": (None, [C.c_void_p]),
    "dd_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "dd_model_enable_early_exit": (C.c_int, [C.c_void_p, C.c_int]),
    "dd_forward_early_exit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "dd_early_exit_select": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int64,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dd_ddpm_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "dd_ddpm_step_coef": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float,
                                    C.c_void_p, C.c_int64, C.c_void_p]),
    "dd_affine_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float,
                                 C.c_void_p, C.c_int64, C.c_void_p]),
    "dd_sample_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                 C.c_uint64, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "dd_to_images": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "dd_sample": (C.c_int, [C.c_void_p, C.POINTER(dd_sample_args), C.c_void_p]),
    "dd_sample_affine": (C.c_int, [C.c_void_p, C.POINTER(dd_affine_sample_args), C.c_void_p]),
    "dd_sample_early_exit": (C.c_int, [C.c_void_p, C.POINTER(dd_ee_sample_args), C.c_void_p]),
    "dd_sample_early_exit_real": (C.c_int, [C.c_void_p, C.POINTER(dd_ee_sample_args), C.POINTER(dd_ee_real), C.c_void_p]),
    "dd_forward_guided": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.POINTER(dd_guidance), C.c_void_p,
                                    C.c_int, C.c_void_p]),
    "dd_sample_guided": (C.c_int, [C.c_void_p, C.POINTER(dd_sample_args), C.POINTER(dd_guidance), C.c_void_p]),
    "dd_sample_affine_guided": (C.c_int, [C.c_void_p, C.POINTER(dd_affine_sample_args), C.POINTER(dd_guidance), C.c_void_p]),
    "dd_multistep_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_float] * 6 +
                          [C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "dd_sample_multistep": (C.c_int, [C.c_void_p, C.POINTER(dd_multistep_sample_args), C.c_void_p]),
    "dd_sample_multistep_guided": (C.c_int, [C.c_void_p, C.POINTER(dd_multistep_sample_args), C.POINTER(dd_guidance), C.c_void_p]),
    "dd_forward_autoguided": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.POINTER(dd_autoguidance), C.c_void_p,
                                        C.c_int, C.c_void_p]),
    "dd_sample_autoguided": (C.c_int, [C.c_void_p, C.POINTER(dd_sample_args), C.POINTER(dd_autoguidance), C.c_void_p]),
    "dd_sample_affine_autoguided": (C.c_int, [C.c_void_p, C.POINTER(dd_affine_sample_args), C.POINTER(dd_autoguidance), C.c_void_p]),
    "dd_sample_multistep_autoguided": (C.c_int, [C.c_void_p, C.POINTER(dd_multistep_sample_args), C.POINTER(dd_autoguidance), C.c_void_p]),
    "dd_forward_perturbed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.POINTER(dd_pag), C.c_void_p,
                                       C.c_int, C.c_void_p]),
    "dd_sample_perturbed": (C.c_int, [C.c_void_p, C.POINTER(dd_sample_args), C.POINTER(dd_pag), C.c_void_p]),
    "dd_sample_affine_perturbed": (C.c_int, [C.c_void_p, C.POINTER(dd_affine_sample_args), C.POINTER(dd_pag), C.c_void_p]),
    "dd_sample_multistep_perturbed": (C.c_int, [C.c_void_p, C.POINTER(dd_multistep_sample_args), C.POINTER(dd_pag), C.c_void_p]),
    "dd_known_blend": (C.c_int, [C.c_void_p] * 5 + [C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "dd_sample_region": (C.c_int, [C.c_void_p, C.POINTER(dd_sample_args), C.POINTER(dd_guidance), C.POINTER(dd_autoguidance),
                                   C.POINTER(dd_known_region), C.c_void_p]),
    "dd_sample_affine_region": (C.c_int, [C.c_void_p, C.POINTER(dd_affine_sample_args), C.POINTER(dd_guidance), C.POINTER(dd_autoguidance),
                                          C.POINTER(dd_known_region), C.c_void_p]),
    "dd_sample_multistep_region": (C.c_int, [C.c_void_p, C.POINTER(dd_multistep_sample_args), C.POINTER(dd_guidance),
                                             C.POINTER(dd_autoguidance), C.POINTER(dd_known_region), C.c_void_p]),
    "dd_jump_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_int64, C.c_void_p]),
    "dd_sample_affine_walk": (C.c_int, [C.c_void_p, C.POINTER(dd_affine_sample_args), C.POINTER(dd_guidance), C.POINTER(dd_autoguidance),
                                        C.POINTER(dd_known_region), C.POINTER(dd_walk), C.c_void_p]),
    "dd_forward_cached": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.POINTER(dd_guidance), C.c_int32, C.c_int32,
                                    C.c_float, C.c_void_p, C.c_int, C.c_void_p]),
    "dd_sample_affine_cached": (C.c_int, [C.c_void_p, C.POINTER(dd_affine_sample_args), C.POINTER(dd_guidance), C.POINTER(dd_known_region),
                                          C.POINTER(dd_block_cache), C.c_void_p]),
    "dd_threshold_step": (C.c_int, [C.c_void_p] * 5 + [C.POINTER(dd_x0_threshold)] + [C.c_float] * 6 +
                          [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "dd_sample_multistep_threshold": (C.c_int, [C.c_void_p, C.POINTER(dd_multistep_sample_args), C.POINTER(dd_guidance),
                                                C.POINTER(dd_autoguidance), C.POINTER(dd_known_region), C.POINTER(dd_x0_threshold), C.c_void_p]),
    "dd_set_image_seeds": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "dd_noise_images": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "dd_scan_error": (C.c_int, [C.c_void_p, C.POINTER(dd_scan_args), C.c_void_p]),
    "dd_scan_error_early_exit": (C.c_int, [C.c_void_p, C.POINTER(dd_scan_exits_args), C.c_void_p]),
    "dd_bench_gemm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_double)]),
    "dd_vae_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "dd_vae_set_param": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int]),
    "dd_vae_finalize": (C.c_int, [C.c_void_p, C.c_int]),
    "dd_vae_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "dd_vae_destroy": (None, [C.c_void_p]),
    "dd_vae_has_encoder": (C.c_int, [C.c_void_p]),
    "dd_vae_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "dd_vae_sample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "dd_profile_steps": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                   C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "dd_profile_steps_chained": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                           C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "dd_profile_select": (C.c_int, [C.c_void_p, C.c_int]),
    "dd_dev_qkv_attention": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_int, C.c_void_p, C.POINTER(C.c_float)]),
    "dd_dev_qkv_attention_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_void_p, C.POINTER(C.c_float)]),
    "dd_dev_v_identity": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_void_p, C.POINTER(C.c_float)]),
    "dd_dev_v_copy": (C.c_int, [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 2 + [C.c_int, C.c_void_p, C.POINTER(C.c_float)]),
    "dd_dev_mlp": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 10 + [C.c_int, C.c_void_p, C.POINTER(C.c_float)] + [C.c_void_p] * 8),
    "dd_dev_block_tail": (C.c_int, [C.c_void_p] + [C.c_int] * 7 + [C.c_void_p] * 21 + [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_float)]),
    "dd_dev_block_tail_frag": (C.c_int, [C.c_void_p] + [C.c_int] * 7 + [C.c_void_p] * 21 + [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_float)] + [C.c_void_p] * 5),
    "dd_dev_qkv_attention_frag": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 7 + [C.c_int, C.c_void_p, C.POINTER(C.c_float)]),
    "dd_dev_head_dec": (C.c_int, [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 9 + [C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_float)]),
    "dd_dev_gemm": (C.c_int, [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 4 + [C.c_int] * 6 + [C.c_void_p] + [C.c_int] * 2 + [C.c_void_p] * 2 +
                    [C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_float)]),
    "dd_dev_rowlin": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 5 + [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_float)]),
    "dd_dev_attention": (C.c_int, [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.POINTER(C.c_float)]),
    "dd_dev_attention_long": (C.c_int, [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.POINTER(C.c_float)]),
    "dd_dev_layernorm": (C.c_int, [C.c_void_p] + [C.c_int] * 3 + [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_void_p, C.POINTER(C.c_float)]),
    "dd_dev_cache_extrapolate": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p,
                                           C.c_int, C.c_void_p, C.POINTER(C.c_float)]),
    "dd_dev_embed": (C.c_int, [C.c_void_p] + [C.c_int] * 9 + [C.c_void_p] * 7 + [C.c_float] + [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.POINTER(C.c_float)]),
    "dd_dev_time_mlp": (C.c_int, [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 6 + [C.c_float, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_float)]),
    "dd_dev_vae_gather": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "dd_dev_groupnorm": (C.c_int, [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 6),
    "dd_dev_softmax_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dd_dev_vae_input": (C.c_int, [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_float, C.c_void_p, C.c_void_p]),
    "dd_dev_vae_output": (C.c_int, [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 3),
    "dd_dev_vae_moments": (C.c_int, [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 7),
    "dd_dev_cast": (C.c_int, [C.c_void_p, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dd_dev_ee_probe": (C.c_int, [C.c_void_p] + [C.c_int] * 7 + [C.c_void_p] * 6),
    "dd_dev_ee_probe_reduce": (C.c_int, [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 3),
    "dd_dev_ee_attn_probe": (C.c_int, [C.c_void_p] + [C.c_int] * 3 + [C.c_void_p] * 10),
    "dd_dev_final": (C.c_int, [C.c_void_p, C.POINTER(dd_dev_final_args), C.c_void_p]),
    "dd_dev_final_seeded": (C.c_int, [C.c_void_p, C.POINTER(dd_dev_final_args), C.c_void_p, C.c_int, C.c_void_p]),
    "dd_dev_scan_diffuse": (C.c_int, [C.c_void_p, C.POINTER(dd_dev_scan_args), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "dd_dev_scan_error": (C.c_int, [C.c_void_p, C.POINTER(dd_dev_scan_args), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "dd_dev_scan_exits_error": (C.c_int, [C.c_void_p, C.POINTER(dd_dev_scan_exits_args)] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 4),
    "dd_dev_poison_workspaces": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "dd_dev_graph_captures": (C.c_longlong, [C.c_void_p]),
    "dd_dev_last_sample_chains": (C.c_int, [C.c_void_p]),
    "dd_dev_ee_real_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong)]),
    "dd_dev_ee_real_cost": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "dd_dev_ee_real_plan": (C.c_int, [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "dd_dev_set_flags": (C.c_int, [C.c_void_p, C.c_uint]),
    "dd_set_num_cus": (C.c_int, [C.c_void_p, C.c_int]),
    "dd_plan_rows": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "dd_last_sample_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
}

_lib = None


class EngineUnavailable(RuntimeError):
    """libduodiff.so is missing or unusable.  There is no CPU path to fall back to."""


def load():
    """dlopen the in-tree library and attach prototypes.  Raises EngineUnavailable if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise EngineUnavailable(
            f"{LIB_PATH} not found: build it with `python -m duodiff_amd.build` "
            "(hipcc --offload-arch=gfx950).  duodiff_amd has no CPU fallback.")
    try:
        lib = C.CDLL(str(LIB_PATH))
    except OSError as e:  # e.g. libamdhip64 missing
        raise EngineUnavailable(f"cannot load {LIB_PATH}: {e}") from e
    lib.dd_abi_version.restype = C.c_int
    if lib.dd_abi_version() != ABI_VERSION:
        raise EngineUnavailable(f"{LIB_PATH}: ABI version {lib.dd_abi_version()}, this package binds version {ABI_VERSION}; rebuild")
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            # the production surface (include/duodiff.h) must be complete; a library built without the development entry
            # points (include/duodiff_dev.h: dd_dev_*), e.g. an A/B build of an older tree, still loads
            if name.startswith("dd_dev_"):
                continue
            raise
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
