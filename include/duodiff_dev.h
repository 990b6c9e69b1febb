/*
 * duodiff_dev.h -- development / validation entry points of libduodiff.so.  NOT part of the drop-in boundary
 * (include/duodiff.h): nothing on the reference side binds these; tests and tools use them to drive one kernel alone.
 */
#ifndef DUODIFF_DEV_H
#define DUODIFF_DEV_H

#include "duodiff.h"
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Development harness for the fused MLP kernel: x += fc2(gelu(fc1(bf16(h)) + b1)) + b2 on host arrays (h [M,D], nn.Linear
 * weights fp32, xres_host [M,D] in/out, out_host optional bf16 copy), plus `iters` timed launches.  extras == 0: the
 * rows are one image of M patch tokens; extras > 0: M / (1 + extras) images of `extras` extra tokens + 1 patch token.
 * ln_in [2, D] (gamma, beta): the kernel's fused-LayerNorm prologue computes h = LayerNorm(xres) itself (h_host is ignored);
 * ln_in NULL: h_host is the (already normalised) input;
 * ln_out [2, D] + ln_out_host [M, D] bf16 or NULL: LayerNorm of the updated rows from the epilogue.
 * ao_host [M, D] + wproj [D, D] + bproj [D] or NULL (needs ln_in, D % 128 == 0): the attention projection
 * x += ao . wproj^T + bproj runs in front of the MLP in the same launch (extra-token rows: the small kernel the model
 * launches for them).
 * skip_host [M, D] + wskip [D, 2D] + bskip [D] or NULL (needs the projection and ln_out): the NEXT block's skip_linear runs
 * behind the MLP in the same launch -- xres_host then receives x' = cat([y, skip]) . wskip^T + bskip instead of y, and
 * ln_out_host its LayerNorm (models/uvit.py:196-200, 206).
 * wqkv [3D, D] + qkv_out_host (bf16, HEAD-MAJOR: [M / L images][3 D / 64 units][Lp = L rounded up to 8][64], L = M for
 * extras == 0, else 1 + extras) or NULL (needs the projection and ln_out): the NEXT block's attn.qkv runs last in the same
 * launch on norm1 of the updated rows (models/uvit.py:152); ln_out_host is then only written for the extra-token rows. */
int dd_dev_mlp(dd_ctx* ctx, int M, int D, int hidden, int extras, const float* h_host, const float* w1, const float* b1,
               const float* w2, const float* b2, float* xres_host, unsigned short* out_host, const float* ln_in,
               const float* ln_out, unsigned short* ln_out_host, int iters, void* stream, float* ms_out,
               const float* ao_host, const float* wproj, const float* bproj, const float* skip_host, const float* wskip,
               const float* bskip, const float* wqkv, unsigned short* qkv_out_host);

/* The block tail as the model launches it (Backbone::block_tail: the fused launch, the reduce launch of the extra-token rows, their skip_linear
 * rows, their qkv rows) on B images of n_patches patch tokens behind `extras` (0, 1 or 2) extra tokens: M = B (extras + n_patches) rows, row plan
 * mlp_fused_plan(B, n_patches, extras, extras + n_patches, hidden).  Modes, each set as the model sets it:
 *   ln_in [2, D] (gamma, beta): norm2 in the prologue, X = nullptr (h_host must be NULL); ln_in NULL: h_host [M, D] is the normalised input;
 *   ao_host [M, D] + wproj [D, D] + bproj [D] (needs ln_in): attn.proj in front, reduce_set = 1;
 *   ln_out [2, D] + ln_out_host (needs ln_in): the next block's norm1 row-major; + frag_host: the patch rows go to frag_host in fragment order
 *     (MlpFusedArgs::ln_out_frag), the reduce launch gets ln_out = nullptr and the skip rows run without their LayerNorm (D = 512);
 *   skip_host [M, D] + wskip [D, 2 D] + bskip [D] (needs the projection, ln_out and out_host): the next block's skip_linear behind the MLP;
 *   tap_host (needs skip): y of every row goes to y_tap before skip_linear replaces it;
 *   wqkv [3 D, D] + qkv_host (needs the projection and ln_out): the next block's attn.qkv last, head-major (images of extras + n_patches rows);
 *   last != 0 (needs the projection; no ln_out / skip / qkv): the last block's launch, n_extra = 0 and tiles_left = 0 after the plan.
 * A combination the launcher refuses is DD_ERR_UNSUPPORTED with nothing launched.
 * Every output array has Mo = round_up(M, 256) + 8 rows of D, is filled with 0xFF bytes before the launch and comes back WHOLE: out_host (the bf16
 * copy), ln_out_host, frag_host (bf16), tap_host (fp32); xres_host [Mo, D] fp32 in / out carries the caller's bytes, canary rows included;
 * qkv_host [(B 3 (D / 64) Lp + 64) 64] bf16; slab_host [slab_rows, D] fp32 or NULL is the kernel's partial-sum buffer, filled with `poison` bytes
 * (slab_rows >= tiles_left groups prows, else DD_ERR_INVALID).  The rows [M, Mo) of the device copies of ao, skip and h hold `poison` in every
 * byte too (0xFF: NaN): the kernel clamps out-of-range rows to row 0 and must never read them.  plan_out[4] (or NULL) receives tiles_main,
 * tiles_left, groups, prows of the launch.  `iters` timed launch sequences -> ms_out. */
int dd_dev_block_tail(dd_ctx* ctx, int B, int n_patches, int extras, int D, int hidden, int last, int poison, const float* h_host,
                      const float* w1, const float* b1, const float* w2, const float* b2, const float* ln_in, const float* ao_host,
                      const float* wproj, const float* bproj, const float* ln_out, const float* skip_host, const float* wskip,
                      const float* bskip, const float* wqkv, float* xres_host, unsigned short* out_host, unsigned short* ln_out_host,
                      unsigned short* frag_host, float* tap_host, unsigned short* qkv_host, float* slab_host, int slab_rows, int* plan_out,
                      int iters, void* stream, float* ms_out);

/* dd_dev_block_tail with the patch rows' hand-offs in MFMA fragment order (embed_dim 512 with the projection in front: MlpFusedArgs::ao_frag,
 * skip_frag, x_in_frag, out_frag, x_out_frag); each of the five is optional, all NULL is dd_dev_block_tail.  A fragment buffer holds the
 * B n_patches patch rows (no extra-token rows, no padding), group = patch row / 32 counted over all images:
 *   bf16 buffers: element ((group (D / 16) + ks) 64 + lane) 8 + j = column 16 ks + 8 (lane >> 5) + j of patch row 32 group + (lane & 31);
 *   fp32 buffers: element (((group (D / 32) + t) 4 + g) 64 + lane) 4 + e = column 32 t + 8 g + 4 (lane >> 5) + e of that row.
 * ao_frag_host / skip_frag_host (bf16 bits) / xin_frag_host (fp32) [B n_patches D]: the main tiles read the patch rows of ao / skip / x from
 * these; the patch rows of the row-major device copies of ao_host / skip_host / xres_host then hold `poison` bytes (the extra-token rows still
 * come from them).  out_frag_host (bf16 bits, needs out_host) / xout_frag_host (fp32) [(B n_patches + 16) D]: the bf16 copy / the updated
 * residual rows of the patch rows go here instead of out_host / xres_host, whose patch rows then keep the bytes they had; both are filled with
 * 0xFF bytes before the launch and come back WHOLE, the data behind 8 canary rows and in front of 8 more. */
int dd_dev_block_tail_frag(dd_ctx* ctx, int B, int n_patches, int extras, int D, int hidden, int last, int poison, const float* h_host,
                           const float* w1, const float* b1, const float* w2, const float* b2, const float* ln_in, const float* ao_host,
                           const float* wproj, const float* bproj, const float* ln_out, const float* skip_host, const float* wskip,
                           const float* bskip, const float* wqkv, float* xres_host, unsigned short* out_host, unsigned short* ln_out_host,
                           unsigned short* frag_host, float* tap_host, unsigned short* qkv_host, float* slab_host, int slab_rows, int* plan_out,
                           int iters, void* stream, float* ms_out, const unsigned short* ao_frag_host, const unsigned short* skip_frag_host,
                           const float* xin_frag_host, unsigned short* out_frag_host, float* xout_frag_host);

/* Development harness for the attention launch that computes attn.qkv itself (attention.hip qkv_attention_kernel; bf16, H heads
 * of 64 with D = 64 H = 512, 768 or 1024, L = 256 patches + `extras` = 1 or 2 leading extra tokens -- qkv_attention_supported; anything else
 * is DD_ERR_UNSUPPORTED): out = softmax(q k^T / 8) v per (image, head) with q, k, v = split(h . wqkv^T + bqkv), from host arrays
 * h [B L, D] (rounded to bf16), wqkv [3 D, D], bqkv [3 D] or NULL; out_host bf16 [B L, D].  `iters` timed launches -> ms_out. */
int dd_dev_qkv_attention(dd_ctx* ctx, int B, int L, int H, int extras, const float* h_host, const float* wqkv, const float* bqkv,
                         unsigned short* out_host, int iters, void* stream, float* ms_out);

/* The same launch with the extra-token rows under the caller's control and every buffer the kernel must leave alone poisoned.
 * xres_host NULL (the hx mode): as dd_dev_qkv_attention, but the patch rows (l >= extras) of the row-major norm1 buffer hold 0xFFFF -- the
 * kernel may read only its rows l < extras.  xres_host [B L, D] fp32 + ln [2, D] (gamma, beta) (the production mode, what the model
 * launches): hx = nullptr, the kernel normalises the extra-token rows itself from the residual stream (norm1, eps 1e-5); only the rows
 * l < extras of xres_host are used, the patch rows of the device copy hold 0xFF bytes (NaN); h_host still supplies the patch rows (its
 * extra-token rows are ignored).  out_host [B L + 8, D] of bf16 bits is filled with 0xFF bytes before the launch and comes back WHOLE.
 * A refused shape is DD_ERR_UNSUPPORTED; nothing is launched and out_host is not written. */
int dd_dev_qkv_attention_rows(dd_ctx* ctx, int B, int L, int H, int extras, const float* h_host, const float* wqkv, const float* bqkv,
                              const float* xres_host, const float* ln, unsigned short* out_host, int iters, void* stream, float* ms_out);

/* dd_dev_qkv_attention_rows with the patch rows' output in fragment order (QkvAttnArgs::out_frag, the layout of the bf16 buffers of
 * dd_dev_block_tail_frag with n_patches = 256): out_frag_host [(B 256 + 16) D] of bf16 bits is filled with 0xFF bytes before the launch and comes
 * back WHOLE, the data behind 8 canary rows and in front of 8 more; out_host [B L + 8, D] then receives the extra-token rows only. */
int dd_dev_qkv_attention_frag(dd_ctx* ctx, int B, int L, int H, int extras, const float* h_host, const float* wqkv, const float* bqkv,
                              const float* xres_host, const float* ln, unsigned short* out_host, unsigned short* out_frag_host, int iters,
                              void* stream, float* ms_out);

/* Development harness for the identity-attention launch (attention.hip v_identity_kernel; perturbed-attention guidance): the companion of the
 * launch above for images whose attention map is the identity, out = v = h . Wv^T + bv with Wv / bv the last third of wqkv / bqkv.  Operands as
 * dd_dev_qkv_attention_rows in its production mode, which is the only one: h_host [B L, D] supplies the patch rows (rounded to bf16; its
 * extra-token rows are ignored), xres_host [B L, D] fp32 + ln [2, D] (gamma, beta) the extra-token rows, which the kernel normalises itself
 * (norm1, eps 1e-5); the patch rows of the device copy of xres hold 0xFF bytes (NaN).  out_host [B L + 8, D] of bf16 bits is filled with 0xFF
 * bytes before the launch and comes back WHOLE.  A refused shape is DD_ERR_UNSUPPORTED; nothing is launched and out_host is not written. */
int dd_dev_v_identity(dd_ctx* ctx, int B, int L, int H, int extras, const float* h_host, const float* wqkv, const float* bqkv,
                      const float* xres_host, const float* ln, unsigned short* out_host, int iters, void* stream, float* ms_out);

/* Development harness for the identity-attention launch of the paths that hold the qkv tensor (attention.hip v_copy_kernel<T>): out = the v
 * rows, bit for bit.  qkv_host: fp32 [B, 3, H, L, 64] (q | k | v per image; precision DD_PREC_BF16: rounded to bf16 here).  The head-major
 * device tensor ([B][3 H][Lp = L rounded up to 8][64] + 64 trailing rows) is filled with 0xFF bytes and only its rows l < L are written: the
 * pad rows hold NaN.  out_host [B L + 8, 64 H] of bf16 bits / fp32 is filled with 0xFF bytes before the launch and comes back WHOLE.  A shape
 * the launcher refuses (L > 288) is DD_ERR_UNSUPPORTED; nothing is launched.  `iters` timed launches -> ms_out. */
int dd_dev_v_copy(dd_ctx* ctx, int precision, int B, int L, int H, const float* qkv_host, void* out_host, int iters, void* stream,
                  float* ms_out);

/* Development harness for the output head's first launch (rowops.hip head_dec_kernel; reference models/uvit.py:377-378):
 * dec = decoder_pred(LayerNorm(x)) in exact fp32 from host arrays x [M, D], norm gamma / beta [D], decoder_pred weight [pd, D] / bias [pd];
 * dec_host [M, pd] (rows the launch does not decode -- the first tok_e rows of every tok_l-row image when tok_l > 0 -- come back as NaN).
 * probe_w [D] + probe_b [1] + srow_host [M] or NULL (D = 256 / 512): the early-exit MLP probe's per-row value sigmoid(x . w + b) from the
 * same launch, for EVERY row (reference models/early_exit.py:31-37).  split != 0 (D = 256 / 512): the product as a split-bf16 product (hi + lo halves,
 * three bf16 MFMAs: 2^-16 of a product; what the bf16 engine's early-exit heads run) instead of the exact fp32 one.  `iters` timed launches -> ms_out. */
int dd_dev_head_dec(dd_ctx* ctx, int M, int D, int pd, int tok_l, int tok_e, const float* x_host, const float* norm_g, const float* norm_b,
                    const float* wdec, const float* bdec, float* dec_host, const float* probe_w, const float* probe_b, float* srow_host,
                    int split, int iters, void* stream, float* ms_out);

/* Development harness for the GEMM path (gemm.hip; what the model's Linears launch): C = [A | A2] . W^T from host arrays -- A [M, K1]
 * (K1 = 0: K), A2 [M, K - K1] or NULL (K1 == K), W [N, K], bias [N] or NULL (NULL: EPI_STORE, or EPI_BIAS_SET without a bias as the KL-VAE's
 * S = Q . K^T launches it; any other epilogue without one is DD_ERR_INVALID); precision DD_PREC_BF16 (operands rounded to bf16: the persistent
 * 256 x 256 kernel where the shape fits it, else the 128 x 128 one; tile128 -1 / 0 / 1 as GemmArgs::tile128) or DD_PREC_FP32 (the exact-f32 parity
 * kernels, 128 x 128 or, N <= 64, 128 x 64).  splits == 0: ONE launch_gemm with `epilogue` (dd_internal.h GemmEpilogue EPI_STORE .. EPI_BIAS_STORE),
 * hm_L > 0: out is written head-major (HeadMajor: images of hm_L rows, hm_H heads, N = 192 hm_H).  splits >= 2 (bf16): the split-K launch into
 * `splits` fp32 slabs, then the reduce_ln row pass (N = 256 .. 1024): x = [x +] sum of slabs + bias (resid), the bf16 copy into out, ln [2, N]
 * (gamma, beta) or NULL: LayerNorm of the updated rows into h_host row-major -- frag_host non-NULL: the patch rows of the tok_l-token images
 * (behind tok_e extra tokens) into frag_host in fragment order (MlpFusedArgs::ln_out_frag) and only the extra-token rows into h_host.
 * Every output array has Mo = round_up(M, 256) + 8 rows and comes back WHOLE: xres_host [Mo, N] fp32 in / out (the caller's bytes go in, canary
 * rows included); out_host [Mo, ldo] (bf16 bits or fp32), head-major [(M / hm_L) 3 hm_H Lp + 64][64]; h_host / frag_host [Mo, N] bf16;
 * slab_host [splits, Mo, N] fp32 (the kernel's slabs are the first splits M N elements) -- filled with 0xFF bytes (NaN) before the launch.
 * num_cus: the CU count the persistent grid is sized for (0: the context's).  `iters` timed launch sequences -> ms_out. */
int dd_dev_gemm(dd_ctx* ctx, int precision, int M, int N, int K, int K1, const float* A, const float* A2, const float* W, const float* bias,
                int epilogue, int tile128, int hm_L, int hm_H, int splits, int resid, const float* ln, int tok_l, int tok_e,
                float* xres_host, void* out_host, int ldo, unsigned short* h_host, unsigned short* frag_host, float* slab_host,
                int num_cus, int iters, void* stream, float* ms_out);

/* Development harness for the row-resident Linear of embed_dim 768 (rowlin.hip rowlin768_kernel, then mlp_reduce_kernel for the K-split
 * extra-token tiles), filled as the model fills them: x = [x +] [A | A2] . W^T + bias (set_x: no residual), W [768, K] packed here as finalize packs
 * it, A [M, lda] / A2 [M, lda] with lda = k_split (k_split > 0: K = 2 k_split, A2 holds k >= k_split) or K.  Rows: B images of n_patches patch
 * tokens behind `extras` extra tokens (M = B (n_patches + extras)), or n_patches == 0: the plain mode over M = B rows.  ln [2, 768] or NULL:
 * LayerNorm of the updated rows into h_host -- row-major, or (frag != 0) the patch rows in fragment order (MlpFusedArgs::ln_out_frag; the extra-token
 * rows' LayerNorm is then not written).  xres_host [Mo, 768] fp32 in / out, x_copy_host (bf16 copy of the updated rows) and h_host [Mo, 768] or
 * NULL, Mo = round_up(M, 256) + 8, returned whole (canary bytes 0xFF before the launch).  `iters` timed launch pairs -> ms_out. */
int dd_dev_rowlin(dd_ctx* ctx, int B, int n_patches, int extras, int K, int k_split, int set_x, const float* A, const float* A2, const float* W,
                  const float* bias, const float* ln, float* xres_host, unsigned short* x_copy_host, unsigned short* h_host, int frag,
                  int iters, void* stream, float* ms_out);

/* Development harness for the plain attention launch (attention.hip attention_kernel<T, 9> for L = 257 / 258, <T, 0> for any other L <= 288;
 * reference models/uvit.py:155-164): out = softmax(q k^T / 8) v per (image, head) from host fp32 q, k, v [B, H, L, 64] (precision DD_PREC_BF16:
 * rounded to bf16 here, so they are exact operands).  The head-major qkv buffer the launch reads ([B][3 H][Lp = L rounded up to 8][64] + 64
 * trailing rows) is filled with 0xFF bytes and only its rows l < L are written: the pad rows [L, Lp), which the qkv Linear never writes, hold
 * NaN.  out_host [B L + 8, 64 H] of bf16 bits / fp32 is filled with 0xFF bytes before the launch and comes back WHOLE.  A shape the launcher
 * refuses (L > 288) is DD_ERR_UNSUPPORTED, L < 1 DD_ERR_INVALID; nothing is launched.  `iters` timed launches -> ms_out. */
int dd_dev_attention(dd_ctx* ctx, int precision, int B, int L, int H, const float* q, const float* k, const float* v, void* out_host,
                     int iters, void* stream, float* ms_out);

/* The same harness for the streaming attention launch of long sequences (attention.hip attention_long_kernel<T>: launch_attention_long; the model
 * takes it where L > 288): the operands, NaN pad rows, canary rows and timing of dd_dev_attention.  It accepts every L the launcher accepts,
 * 1 <= L <= 4098 -- L <= 288 included, so that the two kernels can be compared on the same operands; L > 4098 is DD_ERR_UNSUPPORTED, L < 1
 * DD_ERR_INVALID; nothing is launched. */
int dd_dev_attention_long(dd_ctx* ctx, int precision, int B, int L, int H, const float* q, const float* k, const float* v, void* out_host,
                          int iters, void* stream, float* ms_out);

/* Development harness for the LayerNorm launches (rowops.hip layernorm_kernel<T>): out = LayerNorm(x) gamma + beta (eps 1e-5, biased variance)
 * of host fp32 rows x [rows, D], gamma_beta [2, D].  frag_host NULL: launch_layernorm<T> (T by precision) into out_host, row-major.
 * frag_host non-NULL (bf16 only): launch_layernorm_frag -- the patch rows of the tok_l-token images (behind tok_e extra tokens) go to frag_host in
 * fragment order ([32-row group][D / 16 k-steps][64 lanes] x 8 bf16, MlpFusedArgs::ln_out_frag), only the extra-token rows to out_host.
 * out_host (bf16 bits / fp32) and frag_host have rows + 8 rows of D, are filled with 0xFF bytes before the launch and come back WHOLE.
 * A shape the launcher refuses is DD_ERR_UNSUPPORTED.  `iters` timed launches -> ms_out. */
int dd_dev_layernorm(dd_ctx* ctx, int precision, int rows, int D, const float* x_host, const float* gamma_beta, void* out_host,
                     unsigned short* frag_host, int tok_l, int tok_e, int iters, void* stream, float* ms_out);

/* Development harness for the block cache's kernel (cache.hip cache_extrapolate_kernel<T> through launch_cache_extrapolate; include/duodiff.h
 * dd_block_cache): out = last + w (last - prev) on host rows last_host, prev_host [rows, D] of the activation type (bf16 bits / fp32 by
 * precision), D % 64 == 0.  op 2 extrapolates; op 0 / 1 copy last, and prev's device copy is then never read.  table != 0: the launch's
 * production form -- the op and w travel in row 1 of a device step table (AffineRow::pad1, pad2) whose other rows hold 0xFF bytes, the step state
 * names that row, and the launch's own op / w arguments are -1 / NaN; table == 0: they are the launch's arguments.  out_host [rows + 8, D] is
 * filled with 0xFF bytes before the launch and comes back WHOLE.  out aliases neither input.  `iters` timed launches -> ms_out. */
int dd_dev_cache_extrapolate(dd_ctx* ctx, int precision, int rows, int D, const void* last_host, const void* prev_host, int op, float w,
                             int table, void* out_host, int iters, void* stream, float* ms_out);

/* Development harness for token assembly (rowops.hip embed_kernel / embed_mfma_kernel through launch_embed; reference models/uvit.py:352-365):
 * rows of every image = [label_emb[y],] time sinusoid, (S / P)^2 patch tokens, + pos; L = extras + (S / P)^2, extras = 1 (time) or 2 (label + time).
 * x_img [B, C, S, S], w [D, C, P, P] (transposed here as finalize does), bias [D], pos [L, D], label_emb [num_classes, D] + y [B] (extras == 2),
 * t_vec [B] or NULL: the timestep comes from a device StepState set to t_state (which is set either way).  generic != 0: the VALU kernel even where
 * the MFMA kernel fits.  ln [2, D] (gamma, beta) + ln_frag_host or NULL: the MFMA kernel's variant that also writes the first block's norm1 of the
 * patch rows in fragment order (patch 4, 3 channels, embed_dim 512, not generic; anything else is DD_ERR_UNSUPPORTED).
 * x_tok_host fp32 and ln_frag_host bf16: [Mp + 8, D], Mp = round_up(B L, 256), filled with 0xFF bytes before the launch, returned WHOLE (the
 * launch zeroes rows [B L, Mp)).  `iters` timed launches -> ms_out. */
int dd_dev_embed(dd_ctx* ctx, int B, int C, int S, int P, int D, int extras, int num_classes, int normalize, int generic, const float* x_img,
                 const float* w, const float* bias, const float* pos, const float* label_emb, const long long* y, const float* t_vec,
                 float t_state, const float* ln, float* x_tok_host, unsigned short* ln_frag_host, int iters, void* stream, float* ms_out);

/* Development harness for the time_embed MLP (rowops.hip time_mlp_kernel; reference models/uvit.py:264-272, 358): row extras - 1 of every image of
 * x_tok_host [B L, D] (in / out, returned whole) = w2 . SiLU(w1 . sinusoid(t) + b1) + b2 + pos[extras - 1]; nn.Linear weights w1 [4 D, D], w2 [D, 4 D]
 * (transposed here as finalize does), pos [L, D], t_vec [B] or NULL (the StepState set to t_state).  `iters` timed launches -> ms_out. */
int dd_dev_time_mlp(dd_ctx* ctx, int B, int D, int L, int extras, int normalize, const float* w1, const float* b1, const float* w2,
                    const float* b2, const float* pos, const float* t_vec, float t_state, float* x_tok_host, int iters, void* stream,
                    float* ms_out);

/* Development harness for the two gathers of the KL-VAE encoder (vae_kernels.hip), alone on host arrays.
 * kind 0: Downsample's stride-2 im2col (launch_im2col3x3_s2): src_host = NHWC [B, 2H, 2W, C] elements of `precision` (bf16 bits / fp32),
 *         dst rows = the B H W output pixels, Kpad columns in order (ky, kx, c), columns [9 C, Kpad) zero.
 * kind 1: the encoder's input path (launch_vae_image + launch_im2col3x3_c4): src_host = NCHW fp32 [B, 3, H, W], C is ignored;
 *         dst rows = the B H W pixels, Kpad columns (ky, kx, c of 4) with c = 3 and columns [36, Kpad) zero.
 * kind 2: the 3x3 / pad 1 im2col of the decoder and encoder convolutions (launch_im2col3x3, up = 0): src_host = NHWC [B, H, W, C] elements
 *         of `precision`; rows, columns and padding as kind 0.
 * kind 3: the same through the nearest-2x upsample (up = 1): src_host = NHWC [B, H / 2, W / 2, C], H and W even (else DD_ERR_INVALID).
 * Kpad = 9 C (36 for kind 1) rounded up to the GEMM k-tile of 128 bytes (64 bf16 / 32 fp32 elements), as dd_vae_finalize pads it.
 * dst_host holds dst_bytes >= B H W Kpad elements of `precision`; it is filled with 0xFF bytes before the launch and comes back WHOLE, so
 * the bytes behind the last row keep the canary.  A shape the launcher refuses (kinds 0, 2, 3: C does not fill 16-byte vectors) is
 * DD_ERR_UNSUPPORTED; nothing is launched. */
int dd_dev_vae_gather(dd_ctx* ctx, int kind, int precision, int B, int H, int W, int C, const void* src_host, void* dst_host,
                      size_t dst_bytes, void* stream);

/* Development harnesses for the other kernels of the KL-VAE (vae_kernels.hip), each through its production launch_* function on host arrays.
 * Every output (and the GroupNorm scratch) has DD_DEV_VAE_TAIL elements behind the last one the launch may write; the whole buffer is filled
 * with 0xFF bytes before the launch and comes back WHOLE.  Arguments are checked before anything touches the GPU (DD_ERR_INVALID); a shape
 * the launcher refuses is DD_ERR_UNSUPPORTED and nothing is launched.
 * dd_dev_groupnorm: launch_groupnorm (statistics, finalize, apply): GroupNorm(32 groups, eps 1e-6) [+ x sigmoid(x)] of x_host [B HW, C] fp32
 *   (NHWC) with gamma, beta [C] -> out_host [B HW C + TAIL] of `precision`.  part_host (or NULL): the launch's scratch,
 *   B ceil(HW / 256) 64 + B 64 + TAIL floats (per-chunk partial sums, then (mean, rstd) per (image, group)).  C % 128 != 0 or C > 1024 is refused.
 * dd_dev_softmax_rows: launch_softmax_rows: p = softmax(scale s) over the last dimension of s_host [rows, n] fp32 -> p_host [rows n + TAIL].
 * dd_dev_vae_input: launch_vae_input: z_host [B, 4, HW] -> post_quant_conv(inv_scale z) (w [4, 4], b [4]) -> out_host [B HW 4 + TAIL] (NHWC).
 * dd_dev_vae_output: launch_vae_output: the first C channels of in_host [B HW, ldc] -> out_host [B C HW + TAIL] (NCHW).
 * dd_dev_vae_moments: launch_vae_moments: h_host [B HW, 8] -> quant_conv (w [8, 8], b [8]) -> moments_host [B 8 HW + TAIL] (NCHW) and / or
 *   z_host [B 4 HW + TAIL] = the posterior sample under eps_host [B, 4, HW] (NULL: the mode); either output may be NULL, not both.
 * dd_dev_cast: launch_cast: x_host [n] fp32 -> out_host [n + TAIL] of `precision`. */
#define DD_DEV_VAE_TAIL 64
int dd_dev_groupnorm(dd_ctx* ctx, int precision, int B, int HW, int C, int swish, const float* x_host, const float* gamma, const float* beta,
                     void* out_host, float* part_host, void* stream);
int dd_dev_softmax_rows(dd_ctx* ctx, int precision, int rows, int n, float scale, const float* s_host, void* p_host, void* stream);
int dd_dev_vae_input(dd_ctx* ctx, int B, int HW, const float* z_host, const float* w, const float* b, float inv_scale, float* out_host,
                     void* stream);
int dd_dev_vae_output(dd_ctx* ctx, int B, int C, int HW, int ldc, const float* in_host, float* out_host, void* stream);
int dd_dev_vae_moments(dd_ctx* ctx, int B, int HW, const float* h_host, const float* w, const float* b, const float* eps_host,
                       float* moments_host, float* z_host, void* stream);
int dd_dev_cast(dd_ctx* ctx, int precision, long long n, const float* x_host, void* out_host, void* stream);

/* One GEMM launch of a real KL-VAE decode or encode, copied out as the kernel sees it.  dd_dev_vae_trace runs run_decode (encode == 0:
 * in_dev = z [B, 4, hw, hw], out_dev = images [B, 3, 8 hw, 8 hw]) or run_encode (encode != 0: in_dev = x [B, 3, hw, hw], out_dev = moments
 * [B, 8, hw / 8, hw / 8]) on ONE chunk (B <= max_chunk) of a finalized dd_vae; both are device pointers.  Every GEMM of either direction leaves
 * through one function (vae.hip Net::launch); they are counted in issue order, and launch number `ordinal` is copied to the caller's host
 * buffers around its launch (two stream synchronisations, only in this entry): A [M, K] and W [N, K] elements of the object's precision
 * (bf16 bits / fp32; W is the launch's second operand, whatever it holds), bias [N] fp32 (has_bias == 0: the launch has none, nothing is
 * written), and for the epilogues that write the fp32 stream (EPI_BIAS_SET, EPI_BIAS_RESID) x_before / x_after [M, N] fp32, else out
 * [M, ldo] elements of the precision.  *_bytes are the buffers' capacities; a launch that needs more is DD_ERR_INVALID.  ordinal < 0 (or
 * past the last launch) copies nothing: `launches` and the max_*_bytes any launch of the pass would need come back either way, tapped says
 * whether a launch was copied.  The pass computes what dd_vae_decode / dd_vae_encode compute. */
typedef struct dd_dev_vae_tap {
    int ordinal;
    void *A, *W;
    float *bias, *x_before, *x_after;
    void* out;
    long long a_bytes, w_bytes, bias_bytes, x_bytes, out_bytes;
    int tapped, launches, M, N, K, epilogue, ldo, has_bias;
    long long max_a_bytes, max_w_bytes, max_x_bytes, max_out_bytes;
} dd_dev_vae_tap;
int dd_dev_vae_trace(dd_ctx* ctx, dd_vae* vae, int encode, const float* in_dev, float* out_dev, int B, int hw, dd_dev_vae_tap* tap,
                     void* stream);

/* Development harnesses for the early-exit probes (rowops.hip; reference models/early_exit.py:31-80), each through its production launch_*
 * function on host fp32 arrays.  Every output has DD_DEV_EE_TAIL elements behind the last one the launch may write; the whole buffer is
 * filled with 0xFF bytes before the launch and comes back WHOLE.  Arguments are checked before anything touches the GPU (DD_ERR_INVALID,
 * nothing written).
 * dd_dev_ee_probe: launch_ee_probe as forward.hip calls it: x_host [B L, D] token rows, the probe table pw [n_probe, D] / pb [n_probe], the
 *   step state set to t_state (launch_set_state); the launch reads probe row t_state t_mul + add (outside [0, n_probe): DD_ERR_INVALID) ->
 *   srow_host [B L + TAIL] = sigmoid(x_l . w + b) per token row and out_host [B + TAIL] = their mean per image; out_host NULL: the rows-only
 *   form (the model reduces several layers' rows at once behind the last block: dd_dev_ee_probe_reduce).
 * dd_dev_ee_probe_reduce: launch_ee_probe_reduce: srow_host [rows, L] -> out_host [rows + TAIL] = the mean of each row.
 * dd_dev_ee_attn_probe: launch_ee_attn_probe on x_host [B L, D] with an AttentionProbe's RAW parameters -- q [D], weight_kv wkv [2 D, D] /
 *   bkv [2 D], classification.0 w0 [D, D] / b0 [D], classification.2 w2 [D] / b2 [1] -- folded by the host function finalize folds the
 *   model's probes with (launch_args.h fold_attn_probe) -> out_host [B + TAIL].  L < 2 or D % 64 != 0: DD_ERR_INVALID; more than 64 KB of
 *   LDS (L + 3 D floats): DD_ERR_UNSUPPORTED. */
#define DD_DEV_EE_TAIL 64
int dd_dev_ee_probe(dd_ctx* ctx, int B, int L, int D, int n_probe, int t_state, int t_mul, int add, const float* x_host, const float* pw,
                    const float* pb, float* srow_host, float* out_host, void* stream);
int dd_dev_ee_probe_reduce(dd_ctx* ctx, int rows, int L, const float* srow_host, float* out_host, void* stream);
int dd_dev_ee_attn_probe(dd_ctx* ctx, int B, int L, int D, const float* x_host, const float* q, const float* wkv, const float* bkv,
                         const float* w0, const float* b0, const float* w2, const float* b2, float* out_host, void* stream);

/* Development harness for the launch that ends every sampling step and every forward (step.hip final_tiled_kernel through launch_final:
 * unpatchify, the 3x3 conv, guidance, the step update of step_update.h): ONE launch, from a FinalArgs filled the way forward.hip fills it.
 * All arrays are host fp32.  Geometry: B images of C x S x S (the grid), patches of P, L = extras + (S / P)^2 decoder rows per image, b0 the
 * launch's first image within the whole batch (Philox pixel ids only); `images` >= B (>= 2 pair_B): how many images eps_out, x_in / x_out and h hold.
 * Sources: dec [B L, P P C] ([2 pair_B L, ...] under classifier-free guidance, pair_B == B: image b's unconditional rows at b + pair_B), wconv / bconv
 * (layer_B > 0: the B images are B / layer_B early-exit layers of layer_B images, layer i convolving with wconv + i w_stride / bconv + i b_stride);
 * autoguidance (pair_B == 0): dec2 [B L2, P P C] with its own L2 / extras2 and conv wconv2 / bconv2; guide_scale for either guidance.
 * What the launch is handed: write_eps -> eps_out, write_x -> x_in and x_out (x_alias != 0: the one buffer, as in production; else two), hist_row -> h,
 * known -> kx0 [B, C, S, S] and kmask [B, 1, S, S], noise_mode 1 -> z [B, C, S, S].  eps_out, x_out: [images C S S + 8]; h: [images C S S + 8] in / out
 * (the caller's bytes go in, the 8 trailing elements included; h given without hist_row is handed to the launch beside a null table).  Every output
 * buffer is filled with 0xFF bytes before the launch (x_alias: x_in's `images` images, then 8 canary elements) and comes back WHOLE; a buffer the
 * launch is not handed (write_eps / write_x clear) comes back as the 0xFF it was filled with.
 * The step state is created on the device with t (= t_final), seed and t_model = (float)t or the row's; t_out, t_model_out, t_final_out and seed_out
 * are read back after the launch.  The rule: table == 0, DDPM -- coef at row t of a 1000-row table whose other rows are NaN, `variance`
 * (DD_VAR_*); table != 0 -- the AffineRow of step k = t (row_*) in a table of k + 2 rows, row k + 1 holding next_t_model, every other row and
 * field 0xFF bytes; hist_row: the HistRow of step k (hist_d, hist_p, hist_q, hist) likewise (needs table, write_x and h); known: the KnownRow
 * (known_ka, known_kb) at the row the rule reads (needs write_x).  noise_mode DD_NOISE_*; advance as FinalArgs::advance.
 * Everything the selected instantiation dereferences is checked first -- C in 1..4, P P C <= 64, S % P == 0, L - extras == (S / P)^2 (and of L2 /
 * extras2), t in 0..999 (DDPM) or 0..65535 (table), B % layer_B == 0, no guidance / history / known region beside layer_B, a buffer for every
 * flag, sizes a test has use for (B <= 4096, S <= 1024, extras <= 64, images <= 2 B + 64 and images C S S <= 2^26, strides <= 2^20) -- and a call
 * that fails a check is DD_ERR_INVALID with nothing launched.  No timing loop: the launch mutates x, h and the step state. */
typedef struct dd_dev_final_args {
    int B, C, S, P, L, extras, b0, images;
    const float *dec, *wconv, *bconv;
    const float *dec2, *wconv2, *bconv2;
    int L2, extras2, pair_B, layer_B;
    long long w_stride, b_stride;
    float guide_scale;
    int write_eps, write_x, x_alias;
    float *eps_out, *x_out;
    const float *x_in, *z;
    int t, advance, noise_mode, variance;
    unsigned long long seed;
    int table;
    float c1, c2, sigma_tilde, sigma_beta;
    float row_t_model, row_a, row_b, row_c;
    int row_noise, row_ctr;
    float next_t_model;
    int hist_row;
    float hist_d, hist_p, hist_q;
    int hist;
    float* h;
    int known;
    float known_ka, known_kb;
    const float *kx0, *kmask;
    int t_out, t_final_out;
    float t_model_out;
    unsigned long long seed_out;
} dd_dev_final_args;
int dd_dev_final(dd_ctx* ctx, dd_dev_final_args* args, void* stream);
/* dd_dev_final with per-image seeds (include/duodiff.h dd_set_image_seeds; FinalArgs::seeds): seeds_host [n] uint64 are the seeds of the
 * WHOLE batch, n >= b0 + B, so image b of the launch draws under seeds_host[b0 + b] with image-local pixel ids; args->seed is unused by
 * the draw.  NULL, n < 1, n < b0 + B or n > 2^22: DD_ERR_INVALID, nothing launched. */
int dd_dev_final_seeded(dd_ctx* ctx, dd_dev_final_args* args, const uint64_t* seeds_host, int n, void* stream);

/* Development harnesses for the two kernels of the denoising-error scan (scan.hip; include/duodiff.h dd_scan_error), each through its
 * production launch_* function, ONE launch.  The launch covers B images of C x S x S, images [b0, b0 + B) of a whole batch of B_all >= b0 + B.
 * The step state is created on the device with t = t_final = k (the step index, 0..65535), seed, and t_model = the row's; the row table has
 * k + 2 rows, row k holding the caller's coefficients (t_model, ka, kb, tz, t0, tx, ctr), row k + 1 next_t_model, every other row and field
 * 0xFF bytes.  seeds_host [n_seeds] (or NULL, 0): the per-image seeds of the WHOLE batch, n_seeds >= b0 + B.  t_out, t_final_out and
 * t_model_out are read back after the launch.
 * dd_dev_scan_diffuse: x0_host [B, C, S, S] -> xt_host [8 + B C S S + 8], filled with 0xFF bytes before the launch and returned WHOLE (the
 *   data behind 8 canary elements and in front of 8 more).
 * dd_dev_scan_error: x0_host, m_host [B, C, S, S] (their device copies sit between 8 + 8 elements of 0xFF bytes, NaN, which the kernel must
 *   never read) -> err_host [(k + 1) B_all + 8], filled with 0xFF bytes before the launch and returned WHOLE: the launch writes elements
 *   k B_all + b0 .. + B - 1.  advance as FinalArgs::advance.
 * Everything is checked before anything touches the GPU (B in 1..4096, S in 1..4096, b0 >= 0, B_all <= 2^20, (k + 1) B_all <= 2^24,
 * B C S S <= 2^26, n_seeds <= 2^22, iters in 0..10000 and 0 with advance: DD_ERR_INVALID); a shape the launcher refuses (C outside 1..4, C S S > 2^24) is DD_ERR_UNSUPPORTED with
 * nothing launched. */
typedef struct dd_dev_scan_args {
    int B, C, S, b0, B_all, k;
    float t_model, ka, kb, tz, t0, tx;
    int ctr;
    float next_t_model;
    unsigned long long seed;
    int advance;
    int t_out, t_final_out;
    float t_model_out;
    int iters;          /* > 0 (needs advance == 0): `iters` more launches between two events -> ms_out, the mean of one */
    float ms_out;
} dd_dev_scan_args;
int dd_dev_scan_diffuse(dd_ctx* ctx, dd_dev_scan_args* args, const float* x0_host, const uint64_t* seeds_host, int n_seeds, float* xt_host,
                        void* stream);
int dd_dev_scan_error(dd_ctx* ctx, dd_dev_scan_args* args, const float* x0_host, const float* m_host, const uint64_t* seeds_host, int n_seeds,
                      float* err_host, void* stream);

/* Development harness for the early-exit scan's last kernel (scan.hip scan_exits_error_kernel; include/duodiff.h dd_scan_error_early_exit)
 * through launch_scan_exits_error, ONE launch: B images of C x S x S, images [b0, b0 + B) of a whole batch of B_all, `exits` outputs of one
 * forward -- outs_host [exits - 1, B, C, S, S], eps_host [B, C, S, S] (the last exit), cls_host [exits - 1, B]; exits == 1: outs, cls and pred
 * may be NULL.  The step state is created with t = t_final = the TIMESTEP t (0..999), seed and t_model; the row table has 1001 rows of 0xFF
 * bytes of which row t holds the caller's (t_model, ka, kb, tz, t0, tx, ctr, next), row `next` (0..999) next_t_model and row 1000 the
 * counter base ctr - k, so that the launch writes output row k (0..65535, ctr >= k).  Every input's device copy sits between 8 + 8
 * elements of 0xFF bytes, NaN, which the kernel must never read.  mse_host, tgtu_host [(k + 1) exits B_all + 8] and pred_host
 * [(k + 1) (exits - 1) B_all + 8] are filled with 0xFF bytes before the launch and returned WHOLE: the launch writes elements
 * (k exits + l) B_all + b0 .. + B - 1 of the first two and (k (exits - 1) + l) B_all + b0 .. + B - 1 of pred.  advance, seeds, t_out,
 * t_final_out, t_model_out, iters and ms_out as dd_dev_scan_error.  Everything is checked before anything touches the GPU (the limits of
 * dd_dev_scan_error, (k + 1) exits B_all <= 2^24, B C S S exits <= 2^27: DD_ERR_INVALID); C outside 1..4, C S S > 2^24 or exits > 32 is
 * DD_ERR_UNSUPPORTED with nothing launched. */
typedef struct dd_dev_scan_exits_args {
    int B, C, S, exits, b0, B_all, k, t, next;
    float t_model, ka, kb, tz, t0, tx;
    int ctr;
    float next_t_model;
    unsigned long long seed;
    int advance;
    int t_out, t_final_out;
    float t_model_out;
    int iters;
    float ms_out;
} dd_dev_scan_exits_args;
int dd_dev_scan_exits_error(dd_ctx* ctx, dd_dev_scan_exits_args* args, const float* x0_host, const float* outs_host, const float* eps_host,
                            const float* cls_host, const uint64_t* seeds_host, int n_seeds, float* mse_host, float* tgtu_host,
                            float* pred_host, void* stream);

/* Kernel-variant switches for same-process A/B runs (tools/mlp_check.py, tools/all_configs.py).  They act on models
 * FINALIZED after the call (the kernel paths a model takes, the DD_DEV_NO_FRAG_* hand-offs among them) or on launches made after it; the product never sets them and the library
 * reads no environment variable. */
#define DD_DEV_NO_FUSED_MLP 1u      /* keep the fc1 / fc2 GEMM pair + LayerNorm launches instead of the fused block tail */
#define DD_DEV_NO_FUSED_PROJ 2u     /* keep attn.proj as its own GEMM */
#define DD_DEV_NO_FUSED_HEAD 4u     /* keep final LayerNorm + decoder_pred as two launches */
#define DD_DEV_NO_FUSED_SKIP 32u    /* keep skip_linear as its own GEMM + LayerNorm launch */
#define DD_DEV_NO_FUSED_QKV 64u     /* keep attn.qkv as its own GEMM launch */
#define DD_DEV_NO_FUSED_QA 128u     /* keep attn.qkv out of the attention launch (the qkv tensor goes through HBM) */
#define DD_DEV_GENERIC_EMBED 8u     /* generic VALU patch-embed kernel */
#define DD_DEV_MLP_EXTRAS_ONLY 16u  /* dd_dev_mlp: launch the hidden-split (extra-token) workgroups alone */
#define DD_DEV_NO_CHAINS 256u       /* dd_sample: one chain over the whole batch (default: two half-batch chains on two streams for even B >= 32) */
#define DD_DEV_NO_ROWLIN 1024u       /* embed_dim 768: keep mlp.fc2 as a GEMM + LayerNorm launch pair (default: the row-resident launch of rowlin.hip) */
#define DD_DEV_NO_ROWLIN_PROJ 2048u  /* embed_dim 768: keep attn.proj as a GEMM + LayerNorm launch pair */
#define DD_DEV_NO_EMBED_LN 4096u     /* keep the first block's norm1 as its own launch (default: written by the patch-embed launch where it fits) */
#define DD_DEV_NO_SPLITK 8192u       /* small-batch GEMM-path models: keep skip_linear / attn.proj / mlp.fc2 as whole-K GEMMs + LayerNorm launches */
#define DD_DEV_NO_ROWLIN_SKIP 16384u /* embed_dim 768: keep the out-blocks' skip_linear as a GEMM + LayerNorm launch pair */
#define DD_DEV_NO_SPLIT_HEADS 32768u /* early-exit heads of the bf16 engine: keep the exact-fp32 decoder product (default: the split-bf16 product at embed_dim 256 / 512) */
#define DD_DEV_NO_FRAG_AO 65536u     /* embed_dim 512: keep the attention output of the patch rows row-major between the attention launch and the block tail */
#define DD_DEV_NO_FRAG_SKIP 131072u  /* embed_dim 512: keep the long-skip copy of the patch rows row-major between the in-block and the out-block tails */
#define DD_DEV_NO_FRAG_X 262144u     /* embed_dim 512: keep the fp32 residual patch rows row-major between consecutive block tails */
#define DD_DEV_FORCE_CHAINS 512u    /* dd_sample: two half-batch chains for ANY even batch (tests at small batches) */
int dd_dev_set_flags(dd_ctx* ctx, unsigned flags);

/* Number of hipGraph captures dd_sample has made on this context so far (tests: a second call with other tensors of the
 * same shape must not capture again). */
long long dd_dev_graph_captures(dd_ctx* ctx);

/* Fill every activation buffer of model m -- the main workspace and the second chain's (allocated here if dd_sample has not yet) -- with
 * 0xFF bytes (NaN as bf16 and as fp32) ON `stream`.  Tests: a run that follows must equal a run on a fresh model bit for bit, i.e. no kernel
 * may depend on what a buffer held before the launches of the call wrote it (zero-initialised padding, stale slabs). */
int dd_dev_poison_workspaces(dd_ctx* ctx, dd_model* m, void* stream);

/* Number of chains the last dd_sample call on this context ran (1, or 2 half-batch chains on two streams). */
int dd_dev_last_sample_chains(dd_ctx* ctx);

/* The last dd_sample_early_exit_real call on this context: out3 = block-rows run (the sum over steps, chains and blocks of the images the
 * block was launched on), moves made (image slabs copied, per buffer set), compaction launches made. */
int dd_dev_ee_real_stats(dd_ctx* ctx, long long out3[3]);
/* ... and what the exits cost it: the time its calling thread spent waiting for the counts of compaction layers (ms, host clock), the number
 * of such waits, and the bytes its compactions moved. */
int dd_dev_ee_real_cost(dd_ctx* ctx, double* ms_out, long long* waits_out, long long* bytes_out);
/* The hole-fill plan of a compaction on the host (no device, no context): alive [n] -> *keep_out survivors, *n_moves_out moves (source slot,
 * destination slot) in moves_src_dst [2 * (n / 2)] -- the rule the decision kernel applies. */
int dd_dev_ee_real_plan(const int* alive, int n, int* keep_out, int* n_moves_out, int* moves_src_dst);

/* Host-only (no device, no context): entry `index` of the library's kernel tables, one per instantiation of a kernel that needs the dynamic-LDS
 * opt-in -- the kernel's name, the template arguments its dispatcher selects it by (unused slots 0), its workgroup size and the LDS ceiling it is
 * opted in to.  Returns 0, or 1 past the last entry. */
int dd_dev_kernel_table(int index, char family[32], int key[4], int* block, int* lds_max);
/* ... and the predicates that ask those tables which shapes have a kernel: 1 or 0, DD_ERR_INVALID for an unknown predicate. */
#define DD_DEV_SUP_MLP_FUSED 0        /* args: D, hidden */
#define DD_DEV_SUP_HEAD_DEC 1         /* D, pd */
#define DD_DEV_SUP_HEAD_DEC_PROBE 2   /* D */
#define DD_DEV_SUP_QKV_ATTENTION 3    /* D, H, L, extras */
#define DD_DEV_SUP_ROWLIN 4           /* D, K */
#define DD_DEV_SUP_EMBED_MFMA 5       /* P, C, D, S, L, extras */
#define DD_DEV_SUP_EMBED_LN 6         /* P, C, D, S, L, extras */
int dd_dev_kernel_supported(int predicate, const int args[6]);

#ifdef __cplusplus
}
#endif
#endif /* DUODIFF_DEV_H */
