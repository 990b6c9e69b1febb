// Host-side argument builders that the model (capi.hip: Backbone, finalize) and the single-kernel development entry points (dev_harness.hip)
// share: pure functions of their operands, defined once, so that a development entry point launches exactly what the model launches.
// Hidden visibility: nothing here joins the library's dynamic symbol table.  Not included by any kernel translation unit.
#pragma once
#include "dd_internal.h"

#include <vector>

namespace dd {
#pragma GCC visibility push(hidden)

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// head_dec_kernel operands from a head's LayerNorm (gamma, beta) and decoder_pred (W [pd, D], b): wg = W diag(gamma); dc = c [pd] = b + W . beta,
// then the row sums of wg [pd] (the kernel multiplies the un-normalised rows: dec = rstd (wg . d - mean_d wsum) + c, rowops.hip)
inline void fold_head_norm(int D, int pd, const float* wd, const float* bd, const float* ng, const float* nb, std::vector<float>& wg, std::vector<float>& dc) {
    wg.assign((size_t)pd * D, 0.f);
    dc.assign(2 * (size_t)pd, 0.f);
    for (int r = 0; r < pd; ++r) {
        double acc = bd[r], wsum = 0.0;
        for (int k = 0; k < D; ++k) {
            wg[(size_t)r * D + k] = wd[(size_t)r * D + k] * ng[k];
            acc += (double)wd[(size_t)r * D + k] * (double)nb[k];
            wsum += (double)wg[(size_t)r * D + k];
        }
        dc[r] = (float)acc;
        dc[pd + r] = (float)wsum;
    }
}

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
