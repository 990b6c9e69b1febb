/*
 * duodiff.h -- C ABI of libduodiff.so: the MI355X (gfx950) DuoDiff sampling engine.
 *
 * The reference (razvanmatisan/duodiff) is pure Python and has no FFI; its boundary
 * for the hot path is a pair of Python call signatures:
 *
 *     eps = model(x, time_tensor, y)            sampler.py:130-132, ddpm_core.py:150-152
 *     x   = postprocessing(eps, x, t)           sampler.py:133 -> sampler.py:47-56
 *
 * driven 1000 times by get_samples (sampler.py:82-155) with the backbone switch
 * at t == 1000 - t_switch (sampler.py:135-136).  This header is what a ctypes stub
 * on the reference side binds to replace exactly those calls.
 *
 * Conventions
 *   - plain C: pointers, sizes, ints.  No torch / HIP types in signatures; a stream is
 *     passed as void* (a hipStream_t; NULL = the null stream).
 *   - *_dev pointers are DEVICE pointers owned by the caller (e.g. torch-allocated).
 *     Images are fp32 NCHW contiguous, exactly like the reference's tensors.
 *   - every entry returns 0 on success, a negative dd_status on failure; the message is
 *     kept per context (dd_last_error).  No C++ exception and no abort() crosses the ABI.
 *   - a dd_ctx is bound to one device and is not re-entrant; all device work is enqueued
 *     asynchronously on the caller's stream, only dd_sync blocks.
 *   - there is NO CPU fallback: without a usable GPU dd_ctx_create fails.
 */
#ifndef DUODIFF_H
#define DUODIFF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DD_ABI_VERSION 6

typedef struct dd_ctx dd_ctx;
typedef struct dd_model dd_model;

typedef enum dd_status {
    DD_OK = 0,
    DD_ERR_INVALID = -1,      /* bad argument / shape mismatch   (Python: ValueError / RuntimeError) */
    DD_ERR_NOT_FOUND = -2,    /* unknown parameter name          (Python: KeyError)                  */
    DD_ERR_STATE = -3,        /* call order (e.g. forward before finalize)                          */
    DD_ERR_HIP = -4,          /* a HIP runtime call failed                                           */
    DD_ERR_NOMEM = -5,
    DD_ERR_UNSUPPORTED = -6   /* config outside what the kernels implement                          */
} dd_status;

/* U-ViT hyper-parameters: the YAML model_params block (reference configs/uvit_*.yaml,
 * constructor models/uvit.py:229-247). */
typedef struct dd_config {
    int32_t img_size;
    int32_t patch_size;
    int32_t in_chans;
    int32_t embed_dim;
    int32_t depth;
    int32_t num_heads;
    int32_t mlp_ratio;
    int32_t num_classes;          /* <= 0: unconditional */
    int32_t normalize_timesteps;  /* models/uvit.py:352-353 */
    int32_t max_batch;            /* activation workspace is sized for this many images */
    int32_t qkv_bias;             /* attn.qkv = nn.Linear(dim, 3 dim, bias=qkv_bias), models/uvit.py:150 (no shipped YAML sets it) */
    int32_t mlp_time_embed;       /* time_embed = Linear(D,4D) -> SiLU -> Linear(4D,D) on the sinusoid, models/uvit.py:264-272 */
} dd_config;

/* arithmetic mode of the GEMM / attention operands (accumulation, residual stream,
 * LayerNorm, softmax, head and DDPM update are fp32 in both) */
enum { DD_PREC_BF16 = 0, DD_PREC_FP32 = 1 };

/* sigma_t^2: beta-tilde as sampler.py:50, or beta as ddpm_core.py:57,72-75 (default there) */
enum { DD_VAR_BETA_TILDE = 0, DD_VAR_BETA = 1 };

/* where z ~ N(0, I) of the update comes from */
enum { DD_NOISE_NONE = 0, DD_NOISE_BUFFER = 1, DD_NOISE_PHILOX = 2 };

/* ---- context ---------------------------------------------------------------------- */
int dd_abi_version(void);
/* Hash of the sources this library was built from (duodiff_amd/build.py source_id): profile summaries record it, so a
 * counter value is only ever quoted for the build it was measured on.  Static string; needs no GPU. */
const char* dd_build_id(void);
int dd_ctx_create(int device, dd_ctx** out);
void dd_ctx_destroy(dd_ctx* ctx);
const char* dd_last_error(dd_ctx* ctx);            /* valid until the next call on ctx */
int dd_sync(dd_ctx* ctx, void* stream);

/* The five fp32[1000] schedule tables as the engine computes them (must be bit-equal to
 * sampler.py:40-44) plus the three per-step coefficients.  which: 0 betas, 1 alphas,
 * 2 alphas_bar, 3 alphas_bar_previous, 4 betas_tilde (sampler.py order),
 * 5 betas_tilde (ddpm_core.py:68-70 order), 6 c1=sqrt(1/alpha), 7 c2=(1-alpha)/sqrt(1-abar),
 * 8 sigma=sqrt(betas_tilde).  Works without a GPU (host arithmetic only). */
int dd_schedule_table(int which, float* out1000);

/* NoiseScheduler.__init__ (ddpm_core.py:56-70) for any (beta_init, beta_final, beta_steps): torch.linspace / cumprod
 * restated bit for bit; betas_tilde in the ddpm_core rounding order.  Each output holds `steps` floats or is NULL.
 * Host arithmetic only. */
int dd_schedule_build(float beta_init, float beta_final, int steps, float* betas, float* alphas, float* alphas_bar,
                      float* alphas_bar_prev, float* betas_tilde);

/* ---- model: replaces UViT(**model_params) + load_state_dict (sampler.py:271-293) ---- */
/* Limits (DD_ERR_UNSUPPORTED beyond them): head_dim 64, embed_dim <= 1024, in_chans <= 4, patch_size^2 * in_chans <= 64 and
 * (img_size / patch_size)^2 <= 4096 patches.  Above 288 tokens (patches + the time and label tokens) the attention streams its keys; there
 * dd_model_enable_early_exit and the *_perturbed entries answer DD_ERR_UNSUPPORTED, and x0 thresholding keeps its 16384 elements per image. */
int dd_model_create(dd_ctx* ctx, const dd_config* cfg, dd_model** out);
/* name = the reference state_dict key (models/uvit.py:228-336), data = host fp32,
 * shape must match the reference's exactly.  Copies; may be called in any order. */
int dd_model_set_param(dd_model* m, const char* name, const float* host_data,
                       const int64_t* shape, int ndim);
/* all parameters present -> pack into kernel layouts on the device. */
int dd_model_finalize(dd_model* m, int precision);
int64_t dd_model_num_params(const dd_model* m);
void dd_model_destroy(dd_model* m);

/* ---- eps = model(x, t, y)  (models/uvit.py:351-383) --------------------------------- */
/* x_dev [B,C,S,S] fp32; t = the timestep every row of time_tensor holds (sampler.py:130);
 * t_dev: NULL, or the reference's time_tensor itself, [B] fp32 on the device, when rows differ
 * (then t is ignored); y_dev [B] int64 labels or NULL (must be non-NULL iff num_classes > 0,
 * quirk Q5); eps_dev [B,C,S,S] fp32 out. */
int dd_forward(dd_ctx* ctx, dd_model* m, const float* x_dev, float t, const float* t_dev,
               const int64_t* y_dev, float* eps_dev, int B, void* stream);

/* ---- early-exit baseline: EarlyExitUViT (models/early_exit.py:193-324) + eesampler.py ---- */
/* Which uncertainty probe the model carries (early_exit.py:194-204): the three MLPProbe tables (:31-37) or the
 * per-layer AttentionProbe (:40-80, the reference's default classifier_type). */
enum { DD_EE_MLP_PER_LAYER = 0, DD_EE_MLP_PER_TIMESTEP = 1, DD_EE_MLP_PER_LAYER_PER_TIMESTEP = 2, DD_EE_ATTENTION_PROBE = 3 };
/* Call right after dd_model_create.  dd_model_set_param then also takes the EarlyExitUViT state_dict names
 * (U-ViT names WITHOUT the "uvit." prefix, plus "matrix.<key>.classifier.0.{weight,bias}" -- for the attention probe
 * "matrix.<i>.{q, weight_kv.weight, weight_kv.bias, classification.0.weight, classification.0.bias,
 * classification.2.weight, classification.2.bias}" --,
 * "in_blocks_heads.<i>.*", "mid_block_head.*", "out_blocks_heads.<i>.*") and finalize requires all of them. */
int dd_model_enable_early_exit(dd_model* m, int classifier_type);
/* (eps, classifier_outputs, outputs) = EarlyExitUViT.forward(x, timesteps, y) (early_exit.py:270-320).
 * t = int(timesteps[0]) selects the probes; t_dev as in dd_forward.  classifier_dev [depth, B] fp32: the probe
 * of the input of every block; outputs_dev [depth, B, C, S, S] fp32: the OutputHead of the same inputs. */
int dd_forward_early_exit(dd_ctx* ctx, dd_model* m, const float* x_dev, float t, const float* t_dev,
                          const int64_t* y_dev, float* eps_dev, float* classifier_dev, float* outputs_dev,
                          int B, void* stream);
/* eesampler.py:61-71: per sample the first layer whose predicted error is <= threshold (the final output closes the
 * list with error 0; an all-False column selects layer 0 like torch.argmax) -> model_output_dev [B, chw],
 * indices_dev [B] int32 (or NULL), err_mean_dev [depth] = batch mean of classifier_dev rows (or NULL). */
int dd_early_exit_select(dd_ctx* ctx, const float* outputs_dev, const float* eps_dev, const float* classifier_dev,
                         float threshold, int depth, int B, int64_t chw, float* model_output_dev,
                         int32_t* indices_dev, float* err_mean_dev, void* stream);

/* ---- x = postprocessing(eps, x, t)  (sampler.py:47-56 == ddpm_core.py:190-193) ------ */
/* n = number of elements.  z_dev may be NULL (treated as 0); it is ignored when t == 0. */
int dd_ddpm_step(dd_ctx* ctx, const float* x_dev, const float* eps_dev, const float* z_dev,
                 int t, int variance, float* x_out_dev, int64_t n, void* stream);

/* The same update with the three scalars supplied by the caller: x' = c1 * (x - c2 * eps) + sigma * z (z_dev NULL: no
 * noise term), rounded op by op like the reference.  For schedules other than the 1000-step default
 * (NoiseScheduler(beta_steps=...), ddpm_core.py:167-193): the host derives c1 = sqrt(1/alpha_t),
 * c2 = (1-alpha_t)/sqrt(1-alphas_bar_t), sigma = sqrt(sigma_squared_t) from dd_schedule_build's tables. */
int dd_ddpm_step_coef(dd_ctx* ctx, const float* x_dev, const float* eps_dev, const float* z_dev, float c1, float c2,
                      float sigma, float* x_out_dev, int64_t n, void* stream);

/* ---- generic scalar-affine update: out = a*x + b*m + c*z (z_dev may be NULL) ---------- */
/* The form shared by predict_original / predict_previous post-processing (sampler.py:59-79) and a
 * DDIM step (sampler.py:112-120); the host computes a, b, c from the schedule tables. */
int dd_affine_step(dd_ctx* ctx, const float* x_dev, const float* m_dev, const float* z_dev, float a,
                   float b, float c, float* out_dev, int64_t n, void* stream);

/* ---- samples = rearrange((x + 1) / 2, "b c h w -> b h w c")  (sampler.py:145-146) -------- */
/* x_dev [B,C,S,S] fp32 -> images_dev [B,S,S,C] fp32, unclipped like the reference (quirk Q8).  Lets the whole
 * timed region of get_samples (sampler.py:327-345) stay inside the library: no torch op between the last step
 * and the D2H copy / the gather. */
int dd_to_images(dd_ctx* ctx, const float* x_dev, float* images_dev, int B, int C, int S, void* stream);

/* ---- one fused sampling step: x <- step(x, model(x,t,y), t) in place ---------------- */
/* noise_mode DD_NOISE_BUFFER: z_dev [B,C,S,S] supplies z (parity with the torch CPU stream);
 * DD_NOISE_PHILOX: z is generated on the device from (seed, t, element);
 * eps_out_dev (optional) also receives eps. */
int dd_sample_step(dd_ctx* ctx, dd_model* m, float* x_dev, int t, const int64_t* y_dev,
                   int noise_mode, const float* z_dev, uint64_t seed, int variance,
                   float* eps_out_dev, int B, void* stream);

/* ---- the whole loop: get_samples DDPM branch (sampler.py:128-139) ------------------- */
typedef struct dd_sample_args {
    dd_model* first;        /* model used from t = t_start                                    */
    dd_model* late;         /* or NULL; takes over AFTER the step at t == 1000 - t_switch     */
    int32_t t_switch;       /* <= 0: never switch (reference default: inf, quirk Q6)          */
    int32_t t_start;        /* normally 999                                                   */
    int32_t t_end;          /* normally 0 (inclusive)                                         */
    int32_t variance;       /* DD_VAR_*                                                       */
    int32_t noise_mode;     /* DD_NOISE_PHILOX or DD_NOISE_NONE (host noise: use dd_sample_step) */
    int32_t use_graph;      /* 1: capture one hipGraph per backbone and replay it             */
    uint64_t seed;
    const int64_t* y_dev;   /* [B] or NULL                                                    */
    float* x_dev;           /* in: x_T, out: x at t_end, [B,C,S,S] fp32                       */
    int32_t B;
    int32_t reserved;
} dd_sample_args;
int dd_sample(dd_ctx* ctx, const dd_sample_args* args, void* stream);

/* ---- the other loops of get_samples as device-resident loops: DDIM (sampler.py:103-126) and the predict_original /
 * predict_previous parametrisations (:59-79, :128-139).  Every one of them is  x' = a_k x + b_k model(x, t_k) + c_k z  per
 * step with host-computed scalars (duodiff_amd/sampler.py affine_coefficients, from the bit-exact schedule tables); the
 * table lives on the device, the step's last kernel applies row k and advances the device-resident step index, so one
 * captured hipGraph per backbone is replayed n_steps times (use_graph) -- or the same launches are issued eagerly, bit for bit
 * the same results.  z: device Philox (counter = step index) or none. */
typedef struct dd_affine_sample_args {
    dd_model* first;        /* model used from step 0                                                           */
    dd_model* late;         /* or NULL; runs from step index switch_after on                                    */
    int32_t n_steps;        /* number of updates                                                                */
    int32_t switch_after;   /* >= n_steps (or late == NULL): never                                              */
    const float* t;         /* host [n_steps]: the timestep the model sees at step k                            */
    const float* a;         /* host [n_steps]                                                                   */
    const float* b;         /* host [n_steps]                                                                   */
    const float* c;         /* host [n_steps]                                                                   */
    const int32_t* noise;   /* host [n_steps]: != 0: the c z term is added at step k (the reference skips it at its last step) */
    int32_t noise_mode;     /* DD_NOISE_PHILOX or DD_NOISE_NONE (c z never added)                               */
    int32_t use_graph;
    uint64_t seed;
    const int64_t* y_dev;   /* [B] or NULL                                                                      */
    float* x_dev;           /* in / out, [B,C,S,S] fp32                                                         */
    int32_t B;
    int32_t counter_base;   /* Philox counter of step 0 of THIS call: step k draws z with counter counter_base + k and key seed, so a loop cut
                             * into several calls (intermediate saves) with counter_base = steps already done draws the z of one uncut call   */
} dd_affine_sample_args;
int dd_sample_affine(dd_ctx* ctx, const dd_affine_sample_args* args, void* stream);

/* ---- classifier-free guidance (class-conditional models trained with a null class, U-ViT's ImageNet-256 layout) ---- */
/* A guided step runs the backbone on 2 B rows: the B images with their labels (eps_c), then the same images with null_label
 * (eps_u), and the update uses
 *     eps = eps_c + scale * (eps_c - eps_u)      in fp32, in exactly that order: d = eps_c - eps_u; eps = eps_c + scale * d
 * inside the step's last kernel (no extra launch).  The models' max_batch must hold 2 B rows.  When the loop runs as two chains
 * (the decision is made on 2 B rows), the split is by image: an image's conditional and unconditional rows stay in one chain.
 * Philox noise is drawn per image exactly as the unguided loop draws it, so scale 0 reproduces dd_sample / dd_sample_affine with
 * the same labels.  A label equal to null_label simply makes that image unguided (eps_c == eps_u).
 * DDIM and the predict_original / predict_previous parametrisations guide the raw model output with the same rule: for a fixed
 * x_t both outputs are affine in eps, and the weights (1 + scale, -scale) sum to 1, so guiding the output is guiding eps.
 * Every entry returns DD_ERR_INVALID (with dd_last_error) before enqueueing anything when a model is unconditional, null_label is
 * outside [0, num_classes) of a model, 2 B > max_batch, a model carries early-exit heads (not supported with guidance), or
 * scale is not finite. */
typedef struct dd_guidance {
    float scale;            /* eps = eps_c + scale * (eps_c - eps_u), fp32, in that order */
    int32_t null_label;     /* label of the unconditional rows, 0 <= null_label < num_classes */
} dd_guidance;
/* x_dev [B,C,S,S], y_dev [B] int64 (required), eps_dev [B,C,S,S]: the guided eps at timestep t (host-noise loops, parity) */
int dd_forward_guided(dd_ctx* ctx, dd_model* m, const float* x_dev, float t, const int64_t* y_dev, const dd_guidance* g,
                      float* eps_dev, int B, void* stream);
/* dd_sample / dd_sample_affine with guidance; args->B images, args->y_dev required */
int dd_sample_guided(dd_ctx* ctx, const dd_sample_args* args, const dd_guidance* g, void* stream);
int dd_sample_affine_guided(dd_ctx* ctx, const dd_affine_sample_args* args, const dd_guidance* g, void* stream);

/* ---- multistep update (DPM-Solver++(2M), Lu et al. 2022): the affine row plus one history register per image ---------- */
/*     out = a*x + b*m  [+ d*h  if use_hist]  [+ c*z  if z]        h = p*x + q*m     (x, m: this step's inputs)
 * Each product rounded on its own (no FMA contraction), the terms added in exactly this order (dd_affine_step's, extended).  h is
 * not read when use_hist is 0 (the first step, an uninitialised buffer: 0 * NaN would be NaN); it is written on every step.  x_dev and out_dev may alias;
 * h_dev aliases neither.  m: the model output (guided, with guidance).  The host computes the rows (duodiff_amd.sampler). */
int dd_multistep_step(dd_ctx* ctx, const float* x_dev, const float* m_dev, const float* z_dev, float* h_dev, float a, float b,
                      float c, float d, float p, float q, int use_hist, float* out_dev, int64_t n, void* stream);
/* The multistep loop on the device, as dd_sample_affine (same graphs-per-chain driver, Philox counters, backbone switch) with the
 * history term fused into the step's last kernel.  h_dev [B,C,S,S] fp32 is read at the start and written back at the end, so a
 * loop cut into several calls carries its history across the cuts.  DD_ERR_INVALID before anything is enqueued for n_steps < 1,
 * h_dev == NULL, host noise, an early-exit model, and the guided checks (dd_sample_multistep_guided: h holds the B images). */
typedef struct dd_multistep_sample_args {
    dd_model* first;        /* model used from step 0                                                           */
    dd_model* late;         /* or NULL; runs from step index switch_after on                                    */
    int32_t n_steps;
    int32_t switch_after;   /* >= n_steps (or late == NULL): never                                              */
    const float* t;         /* host [n_steps]: the timestep the model sees at step k                            */
    const float* a;         /* host [n_steps]                                                                   */
    const float* b;         /* host [n_steps]                                                                   */
    const float* c;         /* host [n_steps]                                                                   */
    const int32_t* noise;   /* host [n_steps]: != 0: the c z term is added at step k                            */
    int32_t noise_mode;     /* DD_NOISE_PHILOX or DD_NOISE_NONE                                                 */
    int32_t use_graph;
    uint64_t seed;
    const int64_t* y_dev;   /* [B] or NULL                                                                      */
    float* x_dev;           /* in / out, [B,C,S,S] fp32                                                         */
    int32_t B;
    int32_t counter_base;   /* as dd_affine_sample_args                                                         */
    const float* d;         /* host [n_steps]                                                                   */
    const float* p;         /* host [n_steps]                                                                   */
    const float* q;         /* host [n_steps]                                                                   */
    const int32_t* hist;    /* host [n_steps]: != 0: the d h term is added at step k (h never enters x' otherwise) */
    float* h_dev;           /* in / out, [B,C,S,S] fp32: the history register                                  */
} dd_multistep_sample_args;
int dd_sample_multistep(dd_ctx* ctx, const dd_multistep_sample_args* args, void* stream);
int dd_sample_multistep_guided(dd_ctx* ctx, const dd_multistep_sample_args* args, const dd_guidance* g, void* stream);

/* ---- autoguidance (Karras et al. 2024): the main model guided by a weaker model of the same image geometry -------------- */
/* A DuoDiff user holds the pair already: the full U-ViT and the independently trained shallow one.  An autoguided step runs the guide
 * and then the main model on the SAME B rows of x at the same t (nothing is duplicated: B <= max_batch of each model is all that is
 * needed), and the step's last kernel reads both decoder outputs and uses
 *     eps = eps_main + scale * (eps_main - eps_guide)     in fp32, contraction off, in that order: d = eps_main - eps_guide;
 *                                                         eps = eps_main + scale * d   (the rule of dd_guidance)
 * It needs no labels, so unconditional models (CelebA, CIFAR-10) can be guided.  Each model receives labels if and only if it is
 * class-conditional: y_dev is required when either model is conditional (an unconditional guide under a conditional main model simply
 * gets none) and must be NULL when neither is.
 * A step whose running model is the guide model itself (the same dd_model*) is the plain unguided step: the launches and the bits of
 * dd_sample / dd_sample_affine / dd_sample_multistep.  So the DuoDiff call first = shallow, late = full, guide = shallow runs the first
 * t_switch steps unguided -- x up to the switch is byte-identical to the unguided loop's -- and guides the rest with the model that
 * is the "bad version" exactly there.  The guide's identity decides, not its weights: a second dd_model with the same weights goes through
 * the two-model path (and yields the same bits, d being exactly 0).
 * Philox ids, counters, counter_base and the history register h are exactly the unguided loop's (multistep: m in h' = p x + q m is the
 * guided output, as with classifier-free guidance); scale 0 reproduces the unguided loop.  Two half-batch chains are decided on B rows,
 * chain k running on each model's chain-k workspace; captured graphs are keyed on the guide and the bits of the scale.
 * Embed width, depth, head count, num_classes, mlp_time_embed and precision may differ between the two models.
 * Every entry returns DD_ERR_INVALID (with dd_last_error) before anything is enqueued when g or g->guide is NULL, the guide belongs to
 * another context or is not finalized, img_size / patch_size / in_chans differ between the guide and first or late, any of the models
 * carries early-exit heads, scale is not finite, B is outside a model's max_batch, labels are missing or superfluous under the rule
 * above, or (the loops) the noise mode is host noise.  There is no entry point that takes a dd_guidance as well. */
typedef struct dd_autoguidance {
    dd_model* guide;        /* the weaker model; same context, finalized */
    float scale;            /* d = eps_main - eps_guide; eps = eps_main + scale * d, fp32, in that order */
} dd_autoguidance;
/* x_dev [B,C,S,S], y_dev [B] int64 or NULL (rule above), eps_dev [B,C,S,S]: the autoguided eps at timestep t (host-noise loops, parity) */
int dd_forward_autoguided(dd_ctx* ctx, dd_model* m, const float* x_dev, float t, const int64_t* y_dev, const dd_autoguidance* g,
                          float* eps_dev, int B, void* stream);
/* dd_sample / dd_sample_affine / dd_sample_multistep with autoguidance */
int dd_sample_autoguided(dd_ctx* ctx, const dd_sample_args* args, const dd_autoguidance* g, void* stream);
int dd_sample_affine_autoguided(dd_ctx* ctx, const dd_affine_sample_args* args, const dd_autoguidance* g, void* stream);
int dd_sample_multistep_autoguided(dd_ctx* ctx, const dd_multistep_sample_args* args, const dd_autoguidance* g, void* stream);

/* ---- perturbed-attention guidance (PAG; Ahn et al. 2024): one model, no labels, no second model ------------------------------ */
/* A perturbed step runs the backbone on 2 B rows of the same x_t: the B images as they are (eps), then the same images with the
 * self-attention map of the chosen blocks replaced by the identity -- every token attends only to itself, attention(q, k, v) = v
 * (eps_perturbed) -- and the step's last kernel uses
 *     eps = eps + scale * (eps - eps_perturbed)     in fp32, in that order: d = eps - eps_perturbed; eps = eps + scale * d
 *                                                   (the rule of dd_guidance)
 * A mask names blocks by bit: bit i is block i in forward order (in_blocks, mid_block, out_blocks).  Everything but the attention of a
 * masked block (norm1, attn.qkv, attn.proj, the MLP, the long skips) runs unchanged on all 2 B rows; a block that is not masked runs
 * the launches of the unguided forward.  A class-conditional model sees the labels on both halves ([y | y]); an unconditional model
 * takes none.  Mask 0 makes both halves equal (d is exactly 0: the bits of the unguided entry), scale 0 reproduces the unguided loop.
 * Philox ids, counters, counter_base and the multistep history are the unguided loop's; two half-batch chains are decided on the 2 B
 * rows and split by image as under dd_guidance; captured graphs are keyed on both masks and the bits of the scale.
 * Every entry returns DD_ERR_INVALID (with dd_last_error) before anything is enqueued when the struct is NULL, scale is not finite,
 * a mask names a block at or above the depth of its model, 2 B > max_batch, a model carries early-exit heads, first and late are one
 * model with two different masks, labels are missing or superfluous (as the unguided entries), or (the loops) the noise mode is host
 * noise.  There is no entry point that also takes a dd_guidance, dd_autoguidance, dd_known_region or dd_x0_threshold. */
typedef struct dd_pag {
    float scale;             /* d = eps - eps_perturbed; eps = eps + scale * d (the rule of dd_guidance) */
    uint32_t layers_first;   /* blocks of args->first with identity attention */
    uint32_t layers_late;    /* blocks of args->late with identity attention */
} dd_pag;
/* x_dev [B,C,S,S], y_dev [B] int64 or NULL (as dd_forward), eps_dev [B,C,S,S]: the guided eps at timestep t; uses p->layers_first */
int dd_forward_perturbed(dd_ctx* ctx, dd_model* m, const float* x_dev, float t, const int64_t* y_dev, const dd_pag* p, float* eps_dev,
                         int B, void* stream);
/* dd_sample / dd_sample_affine / dd_sample_multistep with perturbed-attention guidance (multistep: h holds the B images) */
int dd_sample_perturbed(dd_ctx* ctx, const dd_sample_args* args, const dd_pag* p, void* stream);
int dd_sample_affine_perturbed(dd_ctx* ctx, const dd_affine_sample_args* args, const dd_pag* p, void* stream);
int dd_sample_multistep_perturbed(dd_ctx* ctx, const dd_multistep_sample_args* args, const dd_pag* p, void* stream);

/* ---- known regions: inpainting and image-to-image starts (RePaint's replacement rule, Lugmayr et al. 2022, without resampling) ---- */
/* After a step has produced x' (at the noise level the step lands on), every pixel is finished from a known image x0 and a mask m:
 *     kn  = ka * x0                      ka, kb: fp32 scalars of the step
 *     if kb != 0:  kn = kn + kb * z2     z2 ~ N(0,1), a draw of its own
 *     x'' = x'                           if m == 0
 *     x'' = m * kn + (1 - m) * x'        otherwise
 * in fp32, contraction off, each product rounded on its own, in exactly that order.  So m == 0 leaves x' bit for bit (whatever x0 holds)
 * and m == 1 with finite x' gives kn.  The mask is shared by a pixel's channels.  The history register of the multistep rule is not
 * touched: h' = p x + q m comes from the step's inputs.
 * For a step that lands on timestep s the host passes ka = sqrt(alphas_bar[s]), kb = sqrt(1 - alphas_bar[s]), and ka = 1, kb = 0 for
 * a step that lands on the final image (duodiff_amd.sampler known_rows): where m == 1 the result then equals x0 exactly.
 * z2 comes from the device Philox generator with the step's key, batch-wide pixel id and counter (counter_base included), exactly as
 * z is drawn, under another stream word: independent of z, and the same for chained, cut and uncut runs.  DD_NOISE_NONE adds no z2.
 * An image-to-image start needs no entry of its own: the caller noises x0 to the first timestep (dd_affine_step) and starts there. */
typedef struct dd_known_region {
    const float* x0_dev;    /* [B,C,S,S] fp32: the known image, in the model's own space */
    const float* mask_dev;  /* [B,1,S,S] fp32 in [0,1]: 1 = known, 0 = generated */
    const float* ka;        /* host [n_steps] (dd_sample: t_start - t_end + 1 rows, row k = step at t_start - k) */
    const float* kb;        /* host [n_steps]; 0: no noise on that step's known pixels */
} dd_known_region;
/* the rule alone, elementwise: out = x'' of x = x'.  z2_dev [B,C,S,S] or NULL (no z2 term); x_dev and out_dev may alias */
int dd_known_blend(dd_ctx* ctx, const float* x_dev, const float* x0_dev, const float* mask_dev, const float* z2_dev, float ka, float kb,
                   float* out_dev, int B, int C, int S, void* stream);
/* dd_sample / dd_sample_affine / dd_sample_multistep with a known region, fused into the step's last kernel.  g and ag are optional
 * (NULL) and exclusive: the loop is then the guided / autoguided one, and under classifier-free guidance both rows of an image get x''.
 * x0 and the mask are copied into the context at every call, so captured graphs are reused across calls with other tensors of the
 * same shape.  DD_ERR_INVALID (with dd_last_error) before anything is enqueued when kr or one of its members is NULL, both g and ag
 * are given, the noise mode is host noise, a model carries early-exit heads, or a check of the plain / guided entry fails. */
int dd_sample_region(dd_ctx* ctx, const dd_sample_args* args, const dd_guidance* g, const dd_autoguidance* ag, const dd_known_region* kr,
                     void* stream);
int dd_sample_affine_region(dd_ctx* ctx, const dd_affine_sample_args* args, const dd_guidance* g, const dd_autoguidance* ag,
                            const dd_known_region* kr, void* stream);
int dd_sample_multistep_region(dd_ctx* ctx, const dd_multistep_sample_args* args, const dd_guidance* g, const dd_autoguidance* ag,
                               const dd_known_region* kr, void* stream);

/* ---- resampling jumps: RePaint's resampling (Lugmayr et al. 2022) and Restart sampling (Xu et al. 2023) in the table-driven loop ---------- */
/* A walk over a plan's timestep grid that may go back up.  Its table has one row per move: a STEP row is dd_sample_affine's row (the model
 * runs at t[k]); a JUMP row (jump[k] != 0) runs no model and noises x forward from the level it has to a higher one,
 *     x' = ja * x + jc * z3        ja = a[k] = sqrt(abar[u] / abar[s]), jc = c[k] = sqrt(1 - abar[u] / abar[s]), b[k] must be 0
 * in fp32, contraction off, each product rounded on its own (duodiff_amd.step_plan jump_coefficients).  Every pixel takes it, the known
 * ones of a region too (a known row of a jump is not read).  z3 comes from the device Philox generator with the key, pixel id and
 * counter of a step's z (the row's index in the whole walk, counter_base included) under a third stream word: z, z2 and z3 of one counter
 * are independent, and chained, cut and uncut runs draw the same.  noise[k] == 0 or DD_NOISE_NONE: no jc z3 term.
 * A jump from below the switch to above it hands the steps back to the first model: late[k] names each step row's model. */
typedef struct dd_walk {
    const int32_t* jump;    /* host [n_steps]: != 0: row k is a jump */
    const int32_t* late;    /* host [n_steps]: 1: step row k runs args->late, 0: args->first (a jump row's entry is not read); may be NULL:
                             * args->switch_after rules, as in dd_sample_affine */
} dd_walk;
/* the jump alone, elementwise on n values: out = ja * x + jc * z (z_dev NULL: ja * x); x_dev and out_dev may alias */
int dd_jump_step(dd_ctx* ctx, const float* x_dev, const float* z_dev, float ja, float jc, float* out_dev, int64_t n, void* stream);
/* dd_sample_affine[_guided | _autoguided | _region] over a walk: g, ag and kr are optional (NULL), g and ag exclusive.  Everything that
 * loop stages is staged as there (per-image seeds, two half-batch chains, graph replay or eager launches, counter_base); a jump replays
 * a small captured graph of its own per chain.  A table may begin or end with a jump row, and a walk may be cut into calls anywhere.
 * DD_ERR_INVALID before anything is enqueued when walk or its jump array is NULL, a jump row has b != 0, late[k] is outside {0, 1} or 1
 * without a late model, both g and ag are given, a model carries early-exit heads, the noise mode is host noise (drive dd_forward,
 * dd_affine_step, dd_known_blend and dd_jump_step), or a check of dd_sample_affine's own fails. */
int dd_sample_affine_walk(dd_ctx* ctx, const dd_affine_sample_args* args, const dd_guidance* g, const dd_autoguidance* ag,
                          const dd_known_region* kr, const dd_walk* walk, void* stream);

/* ---- block caching: the deep blocks' output reused across sampling steps (DeepCache, Ma et al. 2024; order 1: TaylorSeer) ---------- */
/* A U-ViT of depth nb = 2 h + 1 runs blocks 0 .. nb - 1 in forward order (in-blocks, mid, out-blocks).  With 1 <= K = blocks <= h the DEEP
 * blocks are K .. nb - 1 - K; y_deep, the output of block nb - 1 - K, is the x operand of out-block nb - K's skip_linear, whose long-skip
 * operand is block K - 1's output.  A REFRESH step (op 0) is the full forward and stores y_deep in the model's cache: [rows L, D] of the
 * activation type (bf16 / fp32 by precision), one per chain; with order 1 the cache's `last` becomes `prev` first.  A REUSE step runs embed,
 * blocks 0 .. K - 1, then out-block nb - K with y^ for its x operand and on through the head:
 *     op 1:  y^ = last
 *     op 2:  y^ = last + w * (last - prev)      in fp32 as d = last - prev; y^ = last + w * d, contraction off, rounded once to the activation type
 * A row without a prev is an op-1 row: chosen by the op, never by w = 0 (0 * NaN is NaN).  The host computes op and w per step
 * (duodiff_amd.step_plan: refresh every N-th step of a model, w = (t_1 - t_k) / (t_0 - t_1) from the last two refreshes' timesteps).
 * The engine keeps, per model and chain, what its cache holds: K, the backbone rows, the chain's first image and size, and whether prev is
 * set.  That state outlives a call, so a loop cut into several calls continues where the uncut loop would; every other entry point leaves
 * the cache alone. */
typedef struct dd_block_cache {
    int32_t blocks;         /* K */
    int32_t order;          /* 0: op 2 is not allowed; 1: a refresh rotates prev <- last, a reuse step may extrapolate */
    const int32_t* op;      /* host [n_steps]: 0 refresh, 1 reuse, 2 reuse with extrapolation */
    const float* w;         /* host [n_steps]: the extrapolation weight of an op-2 row (other rows: not read by the update) */
} dd_block_cache;
/* One forward on the whole-batch chain's cache (host-noise loops, parity): eps at timestep t under op (0, 1, 2) and w; g: classifier-free
 * guidance or NULL (the cache then holds the 2 B rows).  A refresh here always rotates prev <- last first. */
int dd_forward_cached(dd_ctx* ctx, dd_model* m, const float* x_dev, float t, const int64_t* y_dev, const dd_guidance* g, int32_t blocks,
                      int32_t op, float w, float* eps_dev, int B, void* stream);
/* dd_sample_affine[_guided | _region] with block caching: g and kr are optional (NULL).  Everything that loop stages is staged as there
 * (per-image seeds, two half-batch chains, graph replay or eager launches, counter_base); each model replays a second captured graph for
 * its reuse step, and the graphs are keyed on K and order.
 * DD_ERR_INVALID before anything is enqueued when cache or one of its arrays is NULL, blocks is outside [1, depth / 2] of a model that runs
 * a step, order is outside {0, 1}, an op is outside {0, 1, 2}, an op is 2 under order 0, a model carries early-exit heads, the noise mode
 * is host noise (drive dd_forward_cached + dd_affine_step), or a check of dd_sample_affine's own fails.  DD_ERR_INVALID as well when a
 * reuse row finds no refresh of its model, chain geometry and K in front of it (in this call or left by an earlier one), or an op-2 row
 * no second one: that check needs the chains, so the step table, the per-image seeds and the known rows have by then been copied to the
 * context's own staging buffers; the caller's tensors, the workspaces and the caches are untouched and no graph is captured.
 * What the caches hold changes once the whole loop is enqueued (dd_forward_cached: the refresh's forward).  A call that fails later than
 * these checks leaves the caches it ran on holding nothing: a reuse row on them is refused until they are refreshed. */
int dd_sample_affine_cached(dd_ctx* ctx, const dd_affine_sample_args* args, const dd_guidance* g, const dd_known_region* kr,
                            const dd_block_cache* cache, void* stream);

/* ---- x0 clipping and dynamic thresholding (Ho et al. 2020; Saharia et al. 2022, Imagen; Lu et al. 2022) of the multistep loop ---------- */
/* The multistep row's data prediction x0 = p*x + q*m (its history expression) is pulled back before it drives the update, and the update
 * takes the result xh in m's place: the rows a, b are UNFOLDED (b multiplies xh, not m; duodiff_amd.sampler multistep_coefficients(...,
 * unfolded=True)).  fp32, contraction off, each product rounded on its own, in the order written:
 *     static  (range r > 0):   xh = min(max(x0, -r), r)
 *     dynamic (quantile qt in (0, 1], ceiling s_max >= 1, may be +inf):
 *         v[0 .. n-1] = |x0| of ONE image's n = C*S*S elements, ascending
 *         pos = qt * (n - 1) in double; i = floor(pos); f = (float)(pos - i)
 *         s  = v[i] + f * (v[min(i+1, n-1)] - v[i]);   s = min(max(s, 1), s_max)
 *         xh = min(max(x0, -s), s) / s                  (correctly rounded division)
 *     out = a*x + b*xh [+ d*h if use_hist] [+ c*z if drawn]            h = xh
 * The order statistic is an exact, deterministic selection on the bit patterns of |x0| (+-inf and denormals are ordinary values; results
 * for NaN inputs are unspecified, the call terminates for any bits).  One image is at most 16384 elements (DD_ERR_UNSUPPORTED beyond).
 * A known region finishes out afterwards, unchanged. */
enum { DD_X0_STATIC = 0, DD_X0_DYNAMIC = 1 };
typedef struct dd_x0_threshold {
    int32_t mode;           /* DD_X0_STATIC | DD_X0_DYNAMIC                     */
    float quantile;         /* dynamic: in (0, 1]                               */
    float range;            /* static: > 0, finite                              */
    float s_max;            /* dynamic: >= 1, may be +inf                       */
} dd_x0_threshold;
/* the rule alone on caller buffers [B,C,S,S]: x_dev and out_dev may alias; h_dev (aliasing neither x, m nor out) is read iff use_hist
 * and always written; z_dev NULL: no c*z term */
int dd_threshold_step(dd_ctx* ctx, const float* x_dev, const float* m_dev, const float* z_dev, float* h_dev, const dd_x0_threshold* thr,
                      float a, float b, float c, float d, float p, float q, int use_hist, float* out_dev, int B, int C, int S,
                      void* stream);
/* dd_sample_multistep_region plus thr, on unfolded rows: g, ag and kr are optional (NULL), g and ag exclusive.  Every step's output head
 * writes the (guided) model output to a context-owned scratch image and a second launch, one workgroup per image, finishes the step.
 * Captured graphs are keyed on the mode and the bits of quantile, range and s_max.  DD_ERR_INVALID (with dd_last_error) before anything
 * is enqueued for a NULL thr, an unknown mode, quantile outside (0, 1], range <= 0 or not finite, s_max < 1 or NaN, host noise, an
 * early-exit model, and every check dd_sample_multistep_region makes. */
int dd_sample_multistep_threshold(dd_ctx* ctx, const dd_multistep_sample_args* args, const dd_guidance* g, const dd_autoguidance* ag,
                                  const dd_known_region* kr, const dd_x0_threshold* thr, void* stream);

/* The early-exit baseline's loop (reference eesampler.py:40-89) as a device-resident loop: per step EarlyExitUViT.forward
 * (all heads and probes), the per-sample exit selection with the global threshold, the DDPM update (sigma^2 = beta-tilde)
 * with the selected output; row t of err_dev [1000, depth] (batch-mean predicted error per layer, :70) and of idx_dev
 * [1000, B] (exit layer per sample, :71) is written when the pointer is non-NULL.  One hipGraph for the step, replayed. */
typedef struct dd_ee_sample_args {
    dd_model* model;        /* created with dd_model_enable_early_exit                        */
    float threshold;
    int32_t t_start;        /* normally 999                                                   */
    int32_t t_end;          /* normally 0 (inclusive)                                         */
    int32_t noise_mode;     /* DD_NOISE_PHILOX or DD_NOISE_NONE                               */
    int32_t use_graph;
    int32_t B;
    uint64_t seed;
    const int64_t* y_dev;   /* [B] or NULL                                                    */
    float* x_dev;           /* in / out                                                       */
    float* err_dev;         /* [1000, depth] fp32 or NULL                                     */
    int32_t* idx_dev;       /* [1000, B] int32 or NULL                                        */
} dd_ee_sample_args;
int dd_sample_early_exit(dd_ctx* ctx, const dd_ee_sample_args* args, void* stream);

/* dd_sample_early_exit with the exits TAKEN (an addition to version 6: new symbols, no struct changes).  dd_sample_early_exit, like the
 * reference, only simulates the exit: every image runs every block.  Here an image whose probe at layer l passes the threshold runs no block
 * from the next compaction layer on: the chain's active images are kept as a prefix of its buffers' slots, a decision launch behind every
 * layer's probe records who leaves, and at the layers l with l % compact_every == 0 the surviving images are moved into the holes and block
 * l runs on the survivors alone.  Every image receives, bit for bit, the images and idx_dev rows dd_sample_early_exit gives for the same
 * arguments (a row takes the same kernels in any slot of any batch; noise is drawn by image).
 * The loop runs as eager launches and BLOCKS THE CALLING THREAD: at every compaction layer the host waits for two counts from the device
 * before it can size the next launches.  It captures no graph and replays none; args->use_graph is not read.  Two half-batch chains under
 * dd_sample_early_exit's policy, alternated by the calling thread.
 * DD_ERR_INVALID (with dd_last_error) before anything is enqueued: a NULL real, compact_every < 1, args->err_dev != NULL (the batch mean of
 * a layer's predicted errors does not exist once images have left in front of it), host noise, and every check dd_sample_early_exit makes;
 * DD_ERR_STATE for a model without early exit. */
typedef struct dd_ee_real {
    int32_t compact_every;  /* >= 1: layers l with l % compact_every == 0 compact (1: every layer) */
    int32_t reserved;
} dd_ee_real;
int dd_sample_early_exit_real(dd_ctx* ctx, const dd_ee_sample_args* args, const dd_ee_real* real, void* stream);

/* ---- per-image seeds (version 6 additions: new symbols, no struct changes): image i = f(seed_i), whatever its batch ---- */
/* Plain (the default, every bit as before): the device noise of a call is Philox with key = the call's seed and a pixel id that runs
 * over the WHOLE batch, id = (i S S + y S + x) for pixel (y, x) of image i -- an image's noise depends on where it sits in its batch.
 * Seeded: key = seeds[i], id = y S + x.  The counter word (the DDPM timestep, or counter_base + k of a table-driven loop) and the
 * stream word (z, the known region's z2, x_T) are the same in both.  So image i of a seeded call with seed s draws exactly what the
 * plain call with B = 1 and seed = s draws: any image of a run can be regenerated alone, and a run does not depend on how it was cut
 * into batches or shared among GPUs.
 *
 * dd_set_image_seeds: seeds_dev [n] uint64 on the device stay with the context until cleared (NULL, 0) -- like dd_set_num_cus.  While
 * set, every entry that draws device noise (every dd_sample* loop, dd_sample_early_exit, dd_sample_step with DD_NOISE_PHILOX) takes
 * image i's draws from seeds_dev[i]; the call's own seed is unused; a call with B != n is DD_ERR_INVALID before anything is enqueued.
 * DD_NOISE_BUFFER and DD_NOISE_NONE calls are unaffected.  Under classifier-free and perturbed-attention guidance the seed is the
 * image's, not the backbone row's.  The array is read at every such call (copied on the call's stream into a buffer of the context,
 * which the captured steps read: calls with other seeds replay the same graphs), so it must stay valid while set.
 * NULL with n != 0, a pointer with n == 0 or n < 0: DD_ERR_INVALID. */
int dd_set_image_seeds(dd_ctx* ctx, const uint64_t* seeds_dev, int n);
/* x_T on the device: out_dev [B, C, S, S] (C in 1..4, S in 1..32768), out[b, c, y, x] = component c of the pixel's four normals under
 * (key, id) as above -- seeds_dev [B] given: seeded, else plain under `seed` -- with counter word `counter` (>= 0) and a stream word of
 * its own: independent of every step's z and z2 under the same key.  Independent of dd_set_image_seeds.  A bad argument is
 * DD_ERR_INVALID with nothing launched; B == 0 does nothing. */
int dd_noise_images(dd_ctx* ctx, uint64_t seed, const uint64_t* seeds_dev, int counter, float* out_dev, int B, int C, int S, void* stream);

/* ---- denoising-error scan on real images (version 6 addition: new symbols only) ---------------- */
/* The training loss of the reference (trainer.py:307-352) evaluated per timestep on the caller's images, as one device-resident loop:
 * for step k = 0 .. n_steps - 1 and image i of x0_dev [B, C, S, S] (model space: pixels in [-1, 1], or latents)
 *     z    = the image's Philox draw with counter counter_base + k and a stream word of its own (independent of every sampling draw)
 *     x_t  = ka[k] x0 + kb[k] z                                  (each product rounded on its own, as the known region's rule)
 *     m    = model(x_t, t[k], y)
 *     tgt  = tz[k] z + t0[k] x0 + tx[k] x_t                      predict_noise (1, 0, 0) | predict_original (0, 1, 0) | predict_previous (0, c_clean, c_noisy)
 *     err_dev[k B + i] = (1 / CHW) sum (m - tgt)^2               fp32, in a summation order that depends on (C, S) alone
 * One hipGraph for the step, replayed (use_graph), or the same launches eagerly, bit for bit the same; two half-batch chains as dd_sample.
 * x0_dev is only read; x_t and the model output live in scratch of the context.  Per-image seeds (dd_set_image_seeds) are honoured like
 * in every other draw: an image's numbers then depend on the image and its seed, not on its batch.  duodiff_amd/step_plan.py scan_rows
 * builds the rows from the bit-exact schedule tables.
 * DD_ERR_INVALID (with dd_last_error) before anything is enqueued: a null pointer, n_steps outside [1, 2^20], counter_base outside [0, 2^20],
 * a noise_mode other than DD_NOISE_PHILOX, an early-exit model, labels that do not fit the model, B outside [1, max_batch], image seeds
 * set for another B.  DD_ERR_UNSUPPORTED: in_chans outside 1..4 or more than 2^24 elements per image.  Guidance is not accepted. */
typedef struct dd_scan_args {
    dd_model* model;
    const float* x0_dev;    /* [B,C,S,S] fp32, read only                                                        */
    const int64_t* y_dev;   /* [B] or NULL                                                                      */
    int32_t B;
    int32_t n_steps;
    const float* t;         /* host [n_steps]: the timestep the model sees at step k                            */
    const float* ka;        /* host [n_steps]: x_t = ka x0 + kb z                                               */
    const float* kb;
    const float* tz;        /* host [n_steps]: tgt = tz z + t0 x0 + tx x_t                                      */
    const float* t0;
    const float* tx;
    uint64_t seed;          /* the Philox key (unused while image seeds are set)                                */
    int32_t counter_base;   /* step k draws with counter counter_base + k: repeats pass r n_steps for fresh z   */
    int32_t noise_mode;     /* DD_NOISE_PHILOX                                                                  */
    int32_t use_graph;
    int32_t reserved;
    float* err_dev;         /* out [n_steps, B] fp32                                                            */
} dd_scan_args;
int dd_scan_error(dd_ctx* ctx, const dd_scan_args* args, void* stream);

/* ---- the early-exit form of the scan (version 6 addition: new symbols only) ---------------- */
/* dd_scan_error for a model created with dd_model_enable_early_exit: the same x_t, target and loop, and from the ONE forward of step k
 * every exit's error.  With depth = the model's depth, exit l < depth the head behind block l and exit depth the backbone's output
 * (the reference's L_n_t and u_t_hats, trainer.py:358-398, per timestep and image):
 *     mse_dev   [(k (depth + 1) + l) B + i] = (1 / CHW) sum (o_l - tgt)^2            summed exactly as dd_scan_error sums it
 *     target_dev[(k (depth + 1) + l) B + i] = (1 / CHW) sum tanh|o_l - tgt|          what probe l was trained to predict
 *     pred_dev  [(k depth + l) B + i]       = probe l's prediction (l < depth)       what dd_sample_early_exit compares with its threshold
 * t[k] must be distinct INTEGERS in [0, 999]: the per-timestep probe tables are indexed by them.  Graph replay, half-batch chains and
 * per-image seeds as dd_scan_error; the three result tables live in scratch of the context and are copied out behind the loop.
 * DD_ERR_STATE: a model without early exit.  DD_ERR_INVALID (with dd_last_error) before anything is enqueued: a null pointer, n_steps
 * outside [1, 2^20], counter_base outside [0, 2^20], a noise_mode other than DD_NOISE_PHILOX, a timestep that is no integer, lies outside
 * [0, 999] or occurs twice, labels that do not fit the model, B outside [1, max_batch], image seeds set for another B.
 * DD_ERR_UNSUPPORTED: in_chans outside 1..4, more than 2^24 elements per image or depth + 1 > 32. */
typedef struct dd_scan_exits_args {
    dd_model* model;
    const float* x0_dev;    /* [B,C,S,S] fp32, read only                                                        */
    const int64_t* y_dev;   /* [B] or NULL                                                                      */
    int32_t B;
    int32_t n_steps;
    const float* t;         /* host [n_steps]: distinct integer timesteps in [0, 999]                           */
    const float* ka;        /* host [n_steps]: x_t = ka x0 + kb z                                               */
    const float* kb;
    const float* tz;        /* host [n_steps]: tgt = tz z + t0 x0 + tx x_t                                      */
    const float* t0;
    const float* tx;
    uint64_t seed;
    int32_t counter_base;
    int32_t noise_mode;     /* DD_NOISE_PHILOX                                                                  */
    int32_t use_graph;
    int32_t reserved;
    float* mse_dev;         /* out [n_steps, depth + 1, B] fp32                                                 */
    float* target_dev;      /* out [n_steps, depth + 1, B] fp32                                                 */
    float* pred_dev;        /* out [n_steps, depth, B] fp32                                                     */
} dd_scan_exits_args;
int dd_scan_error_early_exit(dd_ctx* ctx, const dd_scan_exits_args* args, void* stream);

/* ---- KL-VAE decode: autoencoder.decode(x) at sampler.py:141-143 ---------------- */
/* Replaces FrozenAutoencoderKL.decode (models/utils/autoencoder.py:486-490, Decoder :320-449) for the fixed ddconfig of
 * get_autoencoder (:503-516).  Parameters are set by the reference state_dict keys ("decoder.*", "post_quant_conv.*";
 * "encoder.*" / "quant_conv.*" feed the encoder below).  z_dev [B,4,h,h] fp32 latents -> out_dev [B,3,8h,8h] fp32. */
typedef struct dd_vae dd_vae;
int dd_vae_create(dd_ctx* ctx, int max_chunk, int max_latent, dd_vae** out);
int dd_vae_set_param(dd_vae* v, const char* name, const float* host_data, const int64_t* shape, int ndim);
int dd_vae_finalize(dd_vae* v, int precision);
int dd_vae_decode(dd_ctx* ctx, dd_vae* v, const float* z_dev, float* out_dev, int B, int latent_hw, void* stream);
void dd_vae_destroy(dd_vae* v);

/* ---- KL-VAE encode (version 6 addition): pixel images for latent image-to-image and inpainting ---- */
/* Replaces FrozenAutoencoderKL.encode_moments / sample / encode (models/utils/autoencoder.py:468-484, Encoder :203-317).
 * The encoder is built by dd_vae_finalize iff EVERY "encoder.*" / "quant_conv.*" tensor (108 of them) was set; otherwise the
 * object is decode-only and dd_vae_has_encoder returns 0.  An unknown encode-side name or a wrong shape is an error.
 * dd_vae_encode: x_dev [B,3,8h,8h] fp32 in [-1, 1] -> moments_dev [B,8,h,h] (mean | logvar) and / or
 * z_dev [B,4,h,h] = 0.18215 (mean + exp(0.5 clamp(logvar, -30, 20)) eps); either output may be NULL, not both.  eps_dev [B,4,h,h]
 * is the caller's normal draw; NULL selects the mode, z = 0.18215 mean.  B is chunked by max_chunk as in dd_vae_decode.
 * Rejected before anything is enqueued: a decode-only object (DD_ERR_UNSUPPORTED), image_hw not a multiple of 64
 * (DD_ERR_UNSUPPORTED: the latent pixel count must be a multiple of 64, as for decode), image_hw > 8 max_latent, both outputs
 * NULL, B < 1, NULL input (DD_ERR_INVALID).
 * dd_vae_sample: the sample rule alone on moments_dev [B,8,h,h]; bit-identical to what dd_vae_encode writes for the same moments.
 * Encode and decode of one dd_vae share ONE workspace: calls are ordered by the stream they are given; calls on different
 * streams must be ordered by the caller. */
int dd_vae_has_encoder(const dd_vae* v);
int dd_vae_encode(dd_ctx* ctx, dd_vae* v, const float* x_dev, const float* eps_dev, float* moments_dev, float* z_dev, int B,
                  int image_hw, void* stream);
int dd_vae_sample(dd_ctx* ctx, const float* moments_dev, const float* eps_dev, float* z_dev, int B, int latent_hw, void* stream);

/* ---- measurement support ------------------------------------------------------------ */
/* Time `iters` back-to-back launches of the fc1 GEMM (fused bias+GELU epilogue) of model m at batch B with hipEvents
 * on `stream`: the dominant kernel of the two-GEMM MLP path (fp32 mode, D > 512; bf16 models with D <= 512 run the fused
 * MLP kernel instead, timed in context by dd_profile_steps).  Returns average milliseconds per launch in *ms_out and
 * the launch's algorithmic FLOPs. */
int dd_bench_gemm(dd_ctx* ctx, dd_model* m, int B, int iters, void* stream,
                  float* ms_out, double* flops_out);
/* In-context timing of the dominant kernel: runs `steps` eager sampling steps (t = t_start, t_start-1, ...) in place
 * on x_dev with a hipEvent pair recorded on `stream` around EVERY launch of the block's dominant kernel (depth per step)
 * -- the fused block-tail kernel alone (attn.proj + norm2 + fc1 + GELU + fc2 + residual + next norm1 of the patch rows;
 * the small extra-token launches before and after it are OUTSIDE the pair) where the model uses it, else the fc1 GEMM --
 * and returns the average milliseconds per launch: what rocprofv3 --kernel-trace averages for that kernel. */
int dd_profile_steps(dd_ctx* ctx, dd_model* m, float* x_dev, const int64_t* y_dev, int t_start, int steps, int B,
                     void* stream, float* fc1_ms_out, int* launches_out);
/* Which launches the two profile entries bracket (default DD_PROF_DOMINANT; the choice stays with the context).  bench.py selects the
 * kernel with the largest total time in the workload's committed rocprofv3 kernel table (profiles/rNN/kernel_stats*.csv):
 *   DD_PROF_DOMINANT       the fused block tail where the model has one, else the mlp.fc1 GEMM (the round-1..4 behaviour)
 *   DD_PROF_BLOCK_TAIL     mlp_fused_kernel launches only
 *   DD_PROF_FC1            the mlp.fc1 GEMM (gemm256_kernel<bias + GELU>)
 *   DD_PROF_ROWLIN         every row-resident Linear launch (embed_dim 768: attn.proj, mlp.fc2, skip_linear -- one kernel, rowlin768_kernel)
 *   DD_PROF_QKV_ATTENTION  the attn.qkv + attention launch (qkv_attention_kernel), or the plain attention launch
 *   DD_PROF_SPLITK         every split-K GEMM launch (small-batch embed_dim 1024: attn.proj, mlp.fc2, skip_linear -- gemm256_kernel<partial>) */
#define DD_PROF_DOMINANT 0
#define DD_PROF_BLOCK_TAIL 1
#define DD_PROF_FC1 2
#define DD_PROF_ROWLIN 3
#define DD_PROF_QKV_ATTENTION 4
#define DD_PROF_SPLITK 5
int dd_profile_select(dd_ctx* ctx, int kind);
/* The same measurement for the way dd_sample runs an even batch >= 32: TWO half-batch chains (images [0, B/2) on `stream`, the rest on
 * the context's side stream), enqueued eagerly step by step, an event pair around every launch of the dominant kernel in both
 * chains -- each timed launch covers B/2 images and overlaps the other chain's kernels as in the timed loop. */
int dd_profile_steps_chained(dd_ctx* ctx, dd_model* m, float* x_dev, const int64_t* y_dev, int t_start, int steps, int B,
                             void* stream, float* ms_out, int* launches_out);

/* Host-only: the row partition the 256x256 GEMM uses for C[M,N] = A[M,K] W[N,K]^T on `num_cus` CUs:
 * q main tiles of 256 rows + e (<= 8) tail rows per tile; DD_ERR_UNSUPPORTED if the shape falls back
 * to the generic 128x128 kernel.  Needs no GPU. */
int dd_plan_rows(int M, int N, int K, int num_cus, int* q_out, int* e_out);

/* Number of CUs this context's persistent GEMM grids are sized for (default: the device's CU count, rounded down to
 * a multiple of 8; any value is rounded likewise).  For callers that run the engine on a CU-masked stream
 * (hipExtStreamCreateWithCUMask).  Graphs captured by dd_sample are keyed on the value: the next dd_sample re-captures.
 * A context (its step state, staging buffers and model workspaces) serves ONE stream at a time: calls on different
 * streams must be ordered by the caller. */
int dd_set_num_cus(dd_ctx* ctx, int num_cus);

/* Per-step timing of the last dd_sample call, measured with hipEvents on its stream:
 * [0] total ms, [1] ms in first-model steps, [2] ms in late-model steps.  After dd_sample_affine_walk the split is taken in front of
 * the FIRST late step; once a jump has handed the steps back to the first model the two models interleave, and [1] / [2] no longer
 * mean a model's share: only [0] does. */
int dd_last_sample_timing(dd_ctx* ctx, float out3[3]);

#ifdef __cplusplus
}
#endif
#endif /* DUODIFF_H */
