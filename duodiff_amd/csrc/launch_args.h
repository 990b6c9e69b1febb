// What the model (forward.hip: Backbone; model.hip: finalize) and the single-kernel development entry points (dev_harness.hip) share on the host side, each
// defined once, so that a development entry point packs what finalize packs and launches what the model launches: the weight-image packers (the
// fused block tail's image, the transposed embed / time_embed weights, an output head's and an attention probe's folded operands) and the launch plans (the block tail's
// derived arguments, reduce arguments and follow-up launches; the row-resident and split-K row passes).  Callers own operands and buffers only.
// Hidden visibility: nothing here joins the library's dynamic symbol table.  Not included by any kernel translation unit.
#pragma once
#include "dd_internal.h"
#include "host_arena.h"

#include <cmath>
#include <vector>

namespace dd {
#pragma GCC visibility push(hidden)

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// ---- weight images
// The fused block tail's image (MlpImage): attn.proj in front (wproj, or null), the fc1 / fc2 chunk pairs with b1 in accumulator order (b1p; kperm: the
// launch computes norm2 itself), then the NEXT block's skip_linear and attn.qkv (wskip / wqkv, or null); the run-off blocks stay zero
struct TailImage {
    std::vector<unsigned short> img;
    std::vector<float> b1p;
};
inline TailImage pack_tail_image(int D, int hidden, const float* wproj, const float* w1, const float* b1, const float* w2, bool kperm, const float* wskip,
                                 const float* wqkv) {
    const MlpImage im = MlpImage::of(D, hidden, wproj != nullptr, wskip != nullptr, wqkv != nullptr);
    TailImage t{std::vector<unsigned short>(im.bytes() / 2, 0), std::vector<float>(hidden)};
    auto section = [&](size_t block) { return t.img.data() + im.at(block) / 2; };
    if (wproj) mlp_fused_pack_proj(D, wproj, host_f2bf, section(0));
    mlp_fused_pack(D, hidden, w1, b1, w2, kperm, host_f2bf, section(im.mlp), t.b1p.data());
    if (wskip) mlp_fused_pack_skip(D, wskip, host_f2bf, section(im.skip));
    if (wqkv) mlp_fused_pack_rows(D, 3 * D, wqkv, host_f2bf, section(im.qkv));
    return t;
}

// nn.Linear weight [out, in] -> [in, out] (patch_embed.proj, the two time_embed Linears: their kernels' threads run over the output index)
inline std::vector<float> transposed(const float* w, int out, int in) {
    std::vector<float> wt((size_t)in * out);
    for (int o = 0; o < out; ++o) for (int k = 0; k < in; ++k) wt[(size_t)k * out + o] = w[(size_t)o * in + k];
    return wt;
}

// head_dec_kernel operands from a head's LayerNorm (gamma, beta) and decoder_pred (W [pd, D], b): wg = W diag(gamma); dc = c [pd] = b + W . beta,
// then the row sums of wg [pd] (the kernel multiplies the un-normalised rows: dec = rstd (wg . d - mean_d wsum) + c, rowops.hip).  split: and wg
// as hi + lo bf16 halves in the SPLIT kernel's fragment order (wsplit), with dcs = c, then the row sums of hi + lo
struct HeadImage {
    std::vector<float> wg, dc, dcs;
    std::vector<unsigned short> wsplit;
};
inline HeadImage pack_head_image(int D, int pd, const float* wd, const float* bd, const float* ng, const float* nb, bool split) {
    HeadImage h;
    h.wg.assign((size_t)pd * D, 0.f);
    h.dc.assign(2 * (size_t)pd, 0.f);
    for (int r = 0; r < pd; ++r) {
        double acc = bd[r], wsum = 0.0;
        for (int k = 0; k < D; ++k) {
            h.wg[(size_t)r * D + k] = wd[(size_t)r * D + k] * ng[k];
            acc += (double)wd[(size_t)r * D + k] * (double)nb[k];
            wsum += (double)h.wg[(size_t)r * D + k];
        }
        h.dc[r] = (float)acc;
        h.dc[pd + r] = (float)wsum;
    }
    if (split) {
        h.wsplit = std::vector<unsigned short>((size_t)(D / 32) * ((pd + 15) / 16) * 2 * 64 * 8, 0);
        const float* c = h.dc.data();
        h.dcs.assign(c, c + 2 * (size_t)pd);
        pack_head_split(D, pd, h.wg.data(), host_f2bf, h.wsplit.data(), h.dcs.data() + pd);
    }
    return h;
}

// ee_attn_probe_kernel operands from an AttentionProbe's raw parameters (early_exit.py:40-80; one learned query q [D], one head, weight_kv
// [2 D, D] = Wk over Wv, classification.0 w0 [D, D]).  q . (Wk x + bk) = (Wk^T q) . x + const, and the constant cancels in the softmax;
// sum_l p_l (Wv x_l + bv) = Wv (sum_l p_l x_l) + bv.  So the probe needs u = Wk^T q / sqrt(D) (folded here, in double), and Wv /
// classification.0 transposed for coalesced mat-vecs -- never the [L, 2D] kv.
struct AttnProbeFold {
    std::vector<float> u, wvt, w0t;
};
inline AttnProbeFold fold_attn_probe(int D, const float* q, const float* wkv, const float* w0) {
    AttnProbeFold f{std::vector<float>(D), std::vector<float>((size_t)D * D), std::vector<float>((size_t)D * D)};
    const double scale = 1.0 / std::sqrt((double)D);
    for (int k = 0; k < D; ++k) {
        double acc = 0.0;
        for (int j = 0; j < D; ++j) acc += (double)q[j] * (double)wkv[(size_t)j * D + k];
        f.u[k] = (float)(acc * scale);
    }
    for (int j = 0; j < D; ++j)
        for (int k = 0; k < D; ++k) {
            f.wvt[(size_t)k * D + j] = wkv[(size_t)(D + j) * D + k];
            f.w0t[(size_t)k * D + j] = w0[(size_t)j * D + k];
        }
    return f;
}

// ---- the fused block tail (mlp_fused.hip) on B images of n_patches patch tokens behind `extras` extra tokens, width D with H heads
// The caller has set the pointers of `a`: operands, outputs, hand-offs, weights and biases.  Everything that follows from them: the section counts
// of the image, the head-major map of the qkv output, the row plan.  With the projection in front the extra-token rows' projection runs in their
// hidden-split workgroups and the first group's slab carries x + proj(ao) + b (reduce_set).  last: the LAST block's projection / MLP of the
// extra-token rows feed nothing -- the output head decodes the patch rows only (models/uvit.py:377-380 slices the extras off), and those rows' K / V
// went into this block's attention before -- so no proj_rows / hidden-split workgroups / reduce launch for them
inline void block_tail_plan(MlpFusedArgs& a, int B, int n_patches, int extras, int D, int H, int hidden, bool last) {
    a.ldx = D; a.ldo = D;
    a.nproj = a.ao ? D / 32 : 0;
    a.nskip = a.skip ? D / 16 : 0;
    a.nqkv = a.qkv_out ? 3 * D / 32 : 0;
    if (a.nqkv) a.hm = make_head_major(n_patches + extras, H);
    a.reduce_set = a.nproj ? 1 : 0;
    mlp_fused_plan(B, n_patches, extras, n_patches + extras, hidden, a);
    if (last && a.nproj) { a.n_extra = 0; a.tiles_left = 0; }
}
// the reduce launch's arguments (it finishes the extra-token rows: y in fp32 + the bf16 copy): no norm1 rows where a skip_linear follows or the
// consumer normalises them itself (ln_out_frag: the attention launch)
inline MlpFusedArgs block_tail_reduce_args(const MlpFusedArgs& a) {
    MlpFusedArgs fr = a;
    if (a.nskip || a.ln_out_frag) fr.ln_out = nullptr;
    return fr;
}
// what follows the fused launch (launch_mlp_fused stays with the caller): the reduce launch, the extra-token rows' skip_linear + norm1 in one small
// launch (without the LayerNorm, column-split, where the consumer normalises), their qkv last, from the norm1 rows the launch before wrote
inline hipError_t block_tail_finish(const MlpFusedArgs& a, int D, hipStream_t s) {
    hipError_t e = launch_mlp_reduce(block_tail_reduce_args(a), D, s);
    if (e == hipSuccess && a.nskip) e = launch_skip_rows_ln(a, D, s, !a.ln_out_frag);
    if (e == hipSuccess && a.nqkv) e = launch_qkv_rows(a, D, s);
    return e;
}

// ---- the row passes
// Argument filling of the two row-pass variants of an N = D Linear g (Backbone::rowlin_then_reduce / splitk_then_reduce_ln, dd_dev_rowlin /
// dd_dev_gemm).
// (embed_dim 768) the row-resident launch: x = [x +] g + bias (resid), g's bf16 copy, LayerNorm ln_g / ln_b of the updated rows into h_out
// (row-major) or h_frag (the patch rows in fragment order); rows planned as B images of n_patches patch tokens behind `extras` extra tokens, or
// (n_patches == 0) the plain mode: rows [0, g.M) in tiles of 128
inline RowLinArgs rowlin_args(const GemmArgs<bf16_t>& g, int resid, const char* wimg, float* partial, const float* ln_g, const float* ln_b,
                              bf16_t* h_out, bf16_t* h_frag, int B, int n_patches, int extras) {
    RowLinArgs ra{};
    ra.A = g.A; ra.A2 = g.A2; ra.k_split = g.A2 ? g.K1 : 0; ra.set_x = !resid; ra.lda = g.lda; ra.K = g.K;
    ra.wimg = wimg; ra.bias = g.bias; ra.xres = g.xres; ra.x_copy = g.out; ra.partial = partial;
    if (ln_g) {
        ra.ln_g = ln_g; ra.ln_b = ln_b;
        if (h_frag) ra.h_frag = h_frag; else ra.h_out = h_out;
    }
    if (n_patches > 0) rowlin_plan(B, n_patches, extras, n_patches + extras, ra.K, ra);
    else ra.M = g.M;
    return ra;
}
// ... and the launch that finishes its extra-token rows from the K-split slabs (launch_mlp_reduce)
inline MlpFusedArgs rowlin_reduce_args(const RowLinArgs& ra) {
    MlpFusedArgs fr{};
    fr.b2 = ra.bias; fr.xres = ra.xres; fr.partial = ra.partial; fr.out = ra.x_copy; fr.ldo = 768; fr.reduce_set = ra.set_x;
    fr.tok_n = ra.tok_n; fr.tok_e = ra.tok_e; fr.tok_l = ra.tok_l; fr.n_extra = ra.n_extra; fr.tiles_left = ra.tiles_extra;
    fr.groups = ra.groups; fr.prows = 128;
    if (ra.h_out) { fr.ln_out_g = ra.ln_g; fr.ln_out_b = ra.ln_b; fr.ln_out = ra.h_out; }
    return fr;
}
// the row pass behind a split-K launch of g (g.partial / g.splits): the slabs added in ascending order + bias [+ x], g's bf16 copy, LayerNorm into
// h -- with frag, the patch rows of the tok_l-token images into frag and only the extra-token rows into h
inline ReduceLnArgs splitk_reduce_args(const GemmArgs<bf16_t>& g, int resid, const float* ln_g, const float* ln_b, bf16_t* h, bf16_t* frag, int tok_l, int tok_e) {
    return ReduceLnArgs{g.xres, g.partial, (long long)g.M * g.N, g.splits, resid, g.bias, g.out, g.ldo, ln_g, ln_b, h, ln_g ? frag : nullptr,
                        tok_l, tok_e, g.M};
}
#pragma GCC visibility pop
}  // namespace dd
