// One evaluation of the model and one sampling step as sequences of HIP launches: the U-ViT forward (Backbone), the checks of a call, the
// guided / autoguided / perturbed forms of eps = model(x, t), the step that follows it and the staging buffers such calls run on; the dd_forward*
// entry points and dd_sample_step.  Above model.hip, below loops.hip (engine_state.h).
//
// Host-side restatement of: UViT.forward wiring (reference models/uvit.py:337-383), EarlyExitUViT.forward (models/early_exit.py:290-313).
#include "../../include/duodiff.h"
#include "../../include/duodiff_dev.h"
#include "engine_state.h"
#include "launch_args.h"

#include <cmath>

using namespace dd;

namespace dd {
Mods perturbed(const dd_pag* p, const dd_model* late) {
    Mods mo{};
    mo.pag = p; mo.pag_late = late; mo.missing = p ? nullptr : "null dd_pag";
    return mo;
}

// dd_x0_threshold's checks (null: ok) and the kernel's form of it for images of n elements
const char* check_threshold(const dd_x0_threshold* t) {
    if (!t) return "null dd_x0_threshold";
    if (t->mode == DD_X0_STATIC) return t->range > 0.f && std::isfinite(t->range) ? nullptr : "dd_x0_threshold: range must be positive and finite";
    if (t->mode != DD_X0_DYNAMIC) return "dd_x0_threshold: unknown mode";
    if (!(t->quantile > 0.f && t->quantile <= 1.f)) return "dd_x0_threshold: quantile outside (0, 1]";
    if (!(t->s_max >= 1.f)) return "dd_x0_threshold: s_max must be at least 1 (it may be +inf)";
    return nullptr;
}
X0Threshold kernel_threshold(const dd_x0_threshold* t, long long n) {
    if (t->mode == DD_X0_STATIC) return X0Threshold{0, 0, 0.f, t->range, 0.f};
    const double pos = (double)t->quantile * (double)(n - 1);
    const double i = std::floor(pos);
    return X0Threshold{1, (int)i, (float)(pos - i), 0.f, t->s_max};
}
}  // namespace dd

namespace {
Chain whole_batch(dd_ctx* c, dd_model* m) { return Chain{&m->ws[0], c->st[0], c->num_cus, true}; }

// the output head's arguments that the model and the chain determine, for B images whose decoder rows are in dec; a call site sets the rest by name
FinalArgs final_args(const dd_model* m, const Chain& ch, const float* dec, const float* wconv, const float* bconv, int B) {
    FinalArgs fa{};
    fa.dec = dec; fa.wconv = wconv; fa.bconv = bconv;
    fa.st = ch.st; fa.coef = m->ctx->coef;
    fa.B = B; fa.C = m->cfg.in_chans; fa.S = m->cfg.img_size; fa.P = m->cfg.patch_size; fa.L = m->L; fa.extras = m->extras;
    return fa;
}

// ---- the forward: tokens -> blocks -> decoder_pred patches (the chain's dec) -----------------------
// one forward of B rows of chain ch, enqueued on s (Backbone<T>{m, ch, B, s, ee}): the stages of a block each enqueue their launches and
// pass the next one a Handoff
template <typename T>
struct Backbone {
    static constexpr bool bf16 = sizeof(T) == 2;
    dd_model* m;
    const Chain& ch;
    int B;
    hipStream_t s;
    const EeTaps* ee;
    // perturbation record (perturbed-attention guidance): images [pert_first, B) of this forward take the identity for their attention map in
    // the blocks of pert_mask (bit i = block i in forward order); 0: no block, the launches of an unperturbed forward
    int pert_first = 0;
    unsigned pert_mask = 0;
    // block caching (CacheUse; cu.blocks == 0: none, and every launch below is an uncached forward's).  The seam, on refresh and on reuse alike:
    // block nb - 1 - K hands its output to the chain's cache and does not run the next skip_linear in its own launch (a fused launch consumes
    // the patch rows' y without writing them); out-block nb - K runs its skip_linear as a stage of its own, from the cache and from the
    // row-major long-skip copy that in-block K - 1 therefore writes whole (no fragment copy of its patch rows).
    CacheUse cu{};
    // real early exit (real_exit_stage; 0: none, every launch below is run_backbone's): B is the active prefix of a chain whose step started
    // with B_full images.  The taps' tables keep B_full for their layer stride, so no slot of one layer aliases another's, and each layer's
    // taps are finished in ee_taps itself (its unpatchify / conv and its probe reduce on the layer's own slice: the same kernels, per image the
    // same arithmetic as the one batched launch of ee_finish) -- the exit decision behind them cannot wait for the last block.
    int B_full = 0;
    dd_ctx* c = m->ctx;
    const WsPtrs& ws = *ch.ws;
    const int D = m->D, L = m->L, M = B * L, nb = (int)m->blocks.size();
    const int prof = c->prof_kind == DD_PROF_DOMINANT ? ((bf16 && m->fused_mlp) ? DD_PROF_BLOCK_TAIL : DD_PROF_FC1) : c->prof_kind;
    T *h = (T*)ws.h, *ao = (T*)ws.ao, *qkv = (T*)ws.qkv, *hid = (T*)ws.hid, *xb = (T*)ws.xb;
    // Early-exit heads (m->ee_batched): every layer's LayerNorm + decoder_pred launch writes its own slice of a [depth][B L, pd] buffer and every
    // MLP probe's row launch its own [B, L] slice; ONE unpatchify / conv launch and ONE probe reduce launch behind the last block finish all
    // layers (the per-layer arithmetic is unchanged; 2 x 12 launches less on each step's critical path).  The buffers live in the MLP hidden
    // buffer, which the fused block tail never touches.
    float* ee_dec_all = ee && m->ee_batched ? (float*)ws.hid : nullptr;
    const int Bs = B_full ? B_full : B;       // images per layer of the taps' tables
    float* ee_srow_all = ee_dec_all ? ee_dec_all + (size_t)nb * Bs * L * m->pd : nullptr;
    bool ao_in_frag = false;     // norm1_attention -> block_tail of the same block: the patch rows of the attention output are in aofrag
    const BlockCache& bc = m->cache[ch.ws == &m->ws[1] ? 1 : 0];
    const int deep_first = cu.blocks ? cu.blocks : -1, deep_last = cu.blocks ? nb - 1 - cu.blocks : -1;   // the deep range (-1: no caching)
    // in-block bi is the last block in front of the deep range of a reuse pass: the block behind it does not run, so its tail leaves no norm1
    // (and no fragment-order residual rows) for one -- only its long-skip copy is read, by the seam's skip_linear, which sets x
    bool ends_outer(int bi) const { return cu.reuse && bi + 1 == deep_first; }
    // the x operand of out-block deep_last + 1's skip_linear: the chain's cache, or the extrapolation of it
    const T* cached_y() const { return (const T*)(cu.reuse && cu.extrapolate ? bc.yhat : bc.last); }

    // in-context timing (dd_profile_steps): an event on s in front of and behind every launch of the selected kind (DD_TIMED)
    int mark(int kind) {
        if (!m->time_fc1 || kind != prof) return DD_OK;
        while (m->fc1_events.size() < m->fc1_used + 1) {
            hipEvent_t e;
            DD_HIP(c, hipEventCreate(&e));
            m->fc1_events.push_back(e);
        }
        DD_HIP(c, hipEventRecord(m->fc1_events[m->fc1_used++], s));
        return DD_OK;
    }
#define DD_TIMED(kind, expr) \
    do { if (int rc_ = mark(kind)) return rc_; DD_HIP(c, expr); if (int rc_ = mark(kind)) return rc_; } while (0)

    // 128 x 128 or 256 x 256 tiles for a bf16 Linear: decided for the model's max_batch on the context's CU count -- never for the batch (or the
    // chain-halved grid, Chain::cus) of this call, so that a row takes the same kernel alone, in a full batch and in a half-batch chain
    int tile128(int N, int K, int K1) const { return bf16 && gemm_prefers_128(m->cfg.max_batch * L, N, K, K1, c->num_cus) ? 1 : 0; }
    // the long-skip operand of out-block bi: the in-blocks' outputs, last in first out (uvit.py:374-375)
    const T* skip_of(int bi) const { return (const T*)ws.skips[nb - 1 - bi]; }
    // what a row pass that wrote the next block's norm1 leaves: row-major, or (fused_qa) the patch rows in the attention launch's order
    Handoff norm1_written() const { return Handoff{!m->fused_qa, m->fused_qa}; }

    // The two row-pass variants of an N = D Linear g (skip_linear, attn.proj, mlp.fc2): x = [x +] g + bias (resid), g's bf16 copy (g.out), and
    // LayerNorm ln_g / ln_b of the updated rows into h -- under frag the patch rows into hfrag instead, in the order the attention launch loads them.
    // (embed_dim 768) the row-resident launch (rowlin.hip: W image wimg), then the launch that finishes its extra-token rows from the K-split slabs
    // (g.xres is the residual stream ws.x; g.ldo = D)
    int rowlin_then_reduce(const GemmArgs<bf16_t>& g, int resid, const char* wimg, const float* ln_g, const float* ln_b, bool frag) {
        const RowLinArgs ra = rowlin_args(g, resid, wimg, ws.mlp_partial, ln_g, ln_b, (bf16_t*)h, frag ? ws.hfrag : nullptr, B, m->N, m->extras);
        DD_TIMED(DD_PROF_ROWLIN, launch_rowlin(ra, s));
        DD_HIP(c, launch_mlp_reduce(rowlin_reduce_args(ra), D, s));
        return DD_OK;
    }
    // split-K halves into the slabs, then the row pass that adds them (reduce_ln; under frag the extra-token rows' LayerNorm still goes to h)
    int splitk_then_reduce_ln(GemmArgs<bf16_t> g, int resid, const float* ln_g, const float* ln_b, bool frag) {
        g.partial = ws.mlp_partial; g.splits = 2;
        DD_TIMED(DD_PROF_SPLITK, launch_gemm_splitk(g, s, ch.cus));
        DD_HIP(c, launch_reduce_ln(splitk_reduce_args(g, resid, ln_g, ln_b, (bf16_t*)h, frag ? ws.hfrag : nullptr, L, m->extras), D, s));
        return DD_OK;
    }

    int embed(const float* x_img, const float* t_vec, const int64_t* y_dev, Handoff& first) {
        EmbedArgs ea{x_img, m->emb_wt, m->emb_b, m->pos, m->label, (const long long*)y_dev, t_vec, ch.st, ws.x,
                     B, m->cfg.in_chans, m->cfg.img_size, m->cfg.patch_size, D, L, m->extras,
                     m->cfg.num_classes, m->cfg.normalize_timesteps, round_up(M, 256), (c->dev_flags & DD_DEV_GENERIC_EMBED) ? 1 : 0};
        // the first block's norm1 of the patch rows from the embed launch's registers (where the attention launch computes attn.qkv itself and
        // normalises the extra-token rows from the residual stream: the time_embed MLP below only rewrites such a row)
        if constexpr (bf16) {
            if (m->fused_qa && !(c->dev_flags & DD_DEV_NO_EMBED_LN) && embed_ln_supported(ea)) {
                ea.ln_g = m->blocks[0].ln1_g; ea.ln_b = m->blocks[0].ln1_b; ea.ln_frag = ws.hfrag;
                first.frag = true;
            }
        }
        DD_HIP(c, launch_embed(ea, s));
        if (m->tm_w1t) {   // mlp_time_embed: the time token goes through Linear -> SiLU -> Linear (models/uvit.py:264-272, 358)
            TimeMlpArgs ta{m->tm_w1t, m->tm_b1, m->tm_w2t, m->tm_b2, m->pos, t_vec, ch.st, ws.x, B, D, L, m->extras, m->cfg.normalize_timesteps};
            DD_HIP(c, launch_time_mlp(ta, s));
        }
        return DD_OK;
    }

    // output head and uncertainty probe on the INPUT of block bi (for out-blocks: before skip_linear, as the reference taps x before
    // blk(x, skip)); both read the fp32 residual stream.  In- and mid-blocks: on the context's side stream (side = true), beside this block's
    // norm1 / qkv / attention launches (which only read x); the caller joins it before the first launch that writes x (attn.proj).
    // Out-blocks start with skip_linear, which overwrites x: their heads stay in line.
    int ee_taps(int bi, const Handoff& in, bool& side) {
        if (!ee) return DD_OK;
        const HeadW& hd = m->heads[bi];
        const float* xin = (in.skip && ws.ytap) ? ws.ytap : ws.x;
        side = bi <= m->half_depth && ch.ee_fork && c->side && s != c->side;
        hipStream_t hs = side ? c->side : s;
        if (side) {
            DD_HIP(c, hipEventRecord(c->ev_ee_fork, s));
            DD_HIP(c, hipStreamWaitEvent(c->side, c->ev_ee_fork, 0));
        }
        // probe row: layer bi | timestep t | (t, layer): t is read from the step state inside the launch (a captured
        // step replays for every t); dd_forward_early_exit has put int(t) there
        const int t_mul = m->ee_type == DD_EE_MLP_PER_LAYER ? 0 : m->ee_type == DD_EE_MLP_PER_TIMESTEP ? 1 : nb;
        const int add = m->ee_type == DD_EE_MLP_PER_TIMESTEP ? 0 : bi;
        bool probe_done = false;
        if (hd.wg) {   // the head's LayerNorm + decoder_pred in one exact-fp32 launch (the final head's kernel), patch rows only
            HeadDecArgs ha{xin, hd.wg, hd.dc, ee_dec_all ? ee_dec_all + (size_t)bi * Bs * L * m->pd : ws.dec, M, m->pd, (L - m->extras) % 16 == 0 ? L : 0, m->extras};
            if (hd.wsplit) { ha.wg = hd.wsplit; ha.c = hd.dcs; ha.split = 1; }      // (bf16 engine: the split-bf16 product, rowops.hip SPLIT)
            if (ee_srow_all && m->ee_type != DD_EE_ATTENTION_PROBE && head_dec_probe_supported(D)) {   // ... and the MLP probe's per-token values of the same rows
                ha.srow = ee_srow_all + (size_t)bi * Bs * L; ha.pw_base = m->probe_w; ha.pb_base = m->probe_b; ha.st = ch.st; ha.t_mul = t_mul; ha.add = add;
                probe_done = true;
            }
            DD_HIP(c, launch_head_dec(ha, D, ch.cus, hs));
        } else {
            float* hf = (float*)ws.hid;   // the MLP hidden buffer is free between blocks
            DD_HIP(c, launch_layernorm<float>(xin, hd.ng, hd.nb, hf, M, D, hs));
            GemmArgs<float> g{hf, nullptr, hd.wdec, hd.bdec, ws.dec, nullptr, M, m->pd, D, D, D, 0, m->pd};
            DD_HIP(c, launch_gemm<float>(g, EPI_BIAS_SET, hs, ch.cus));
        }
        if (!ee_dec_all) {
            const long long chw = (long long)m->cfg.in_chans * m->cfg.img_size * m->cfg.img_size;
            FinalArgs fa = final_args(m, ch, ws.dec, hd.wconv, hd.bconv, B);
            fa.eps_out = ee->outs + (long long)bi * Bs * chw;
            DD_HIP(c, launch_final(fa, hs));
        }
        if (m->ee_type == DD_EE_ATTENTION_PROBE) {
            DD_HIP(c, launch_ee_attn_probe(xin, m->attn_probes[bi], ee->cls + (long long)bi * Bs, B, L, D, hs));
        } else if (!probe_done) {
            if (ee_srow_all) DD_HIP(c, launch_ee_probe(xin, m->probe_w, m->probe_b, nullptr, ee_srow_all + (size_t)bi * Bs * L, B, L, D, ch.st, t_mul, add, hs));   // rows only: reduced behind the last block
            else DD_HIP(c, launch_ee_probe(xin, m->probe_w, m->probe_b, ee->cls + (long long)bi * Bs, (float*)ws.hid, B, L, D, ch.st, t_mul, add, hs));   // (the MLP hidden buffer is free between blocks)
        }
        if (B_full && ee_dec_all) {      // real early exit: this layer's share of ee_finish, now
            const long long chw = (long long)m->cfg.in_chans * m->cfg.img_size * m->cfg.img_size;
            FinalArgs fa = final_args(m, ch, ee_dec_all + (size_t)bi * Bs * L * m->pd, hd.wconv, hd.bconv, B);
            fa.eps_out = ee->outs + (long long)bi * Bs * chw;
            DD_HIP(c, launch_final(fa, hs));
            if (m->ee_type != DD_EE_ATTENTION_PROBE) DD_HIP(c, launch_ee_probe_reduce(ee_srow_all + (size_t)bi * Bs * L, ee->cls + (long long)bi * Bs, B, L, hs));
        }
        if (side) DD_HIP(c, hipEventRecord(c->ev_ee_join, c->side));
        return DD_OK;
    }

    // out-blocks: x = skip_linear(cat[x, skip]), unless the previous block's fused launch ran it; the row-resident and split-K variants
    // leave this block's norm1 behind
    int skip_linear(int bi, Handoff& hand) {
        if (bi <= m->half_depth || hand.skip) return DD_OK;
        const BlockW& w = m->blocks[bi];
        GemmArgs<T> g{bi == deep_last + 1 ? cached_y() : xb, skip_of(bi), (const T*)w.skip_w, w.skip_b, ws.x, nullptr, M, D, 2 * D, D, D, D, D};
        g.tile128 = tile128(D, 2 * D, D);
        if constexpr (bf16) {
            if (m->rowlin_skip || m->splitk) hand = norm1_written();
            if (m->rowlin_skip) return rowlin_then_reduce(g, 0, w.rls_img, w.ln1_g, w.ln1_b, m->fused_qa);
            if (m->splitk) return splitk_then_reduce_ln(g, 0, w.ln1_g, w.ln1_b, m->fused_qa);
        }
        DD_HIP(c, launch_gemm<T>(g, EPI_BIAS_SET, s, ch.cus));
        return DD_OK;
    }

    // ao = attention(attn.qkv(norm1(x))), norm1 and qkv where the launches in front did not leave them
    int norm1_attention(int bi, const Handoff& in) {
        const BlockW& w = m->blocks[bi];
        bool qa = in.frag;
        if (!in.h && !in.frag && !in.qkv) {
            if (bf16 && m->fused_qa) {
                // (the first block; blocks behind a skip_linear GEMM when that fusion is off) norm1 straight into the order the
                // attention launch loads it, so that these blocks take the same launch as the others
                DD_HIP(c, launch_layernorm_frag(ws.x, w.ln1_g, w.ln1_b, (bf16_t*)h, ws.hfrag, M, D, L, m->extras, s));
                qa = true;
            } else {
                DD_HIP(c, launch_layernorm<T>(ws.x, w.ln1_g, w.ln1_b, h, M, D, s));
            }
        }
        // a masked block: the attention launch on images [0, Bn), the identity launch on the Bi images behind them (operands offset by image)
        const bool masked = (pert_mask >> bi) & 1u;
        const int Bn = masked ? pert_first : B, Bi = B - Bn;
        // the patch rows' output in the order the tail's projection loads it -- not in a block where the identity launch runs: that block takes the
        // row-major ao on both sides
        ao_in_frag = qa && m->frag_ao && Bi == 0;
        if (qa) {
            if constexpr (bf16) {
                if (Bn > 0)
                    DD_TIMED(DD_PROF_QKV_ATTENTION, launch_qkv_attention(ws.hfrag, w.qa_img, w.qkv_b, nullptr, ws.x, w.ln1_g, w.ln1_b, (bf16_t*)ao, Bn, L, m->H, D, m->extras, s,
                                                                         ao_in_frag ? ws.aofrag : nullptr));
                if (Bi > 0)
                    DD_HIP(c, launch_v_identity(ws.hfrag + (size_t)Bn * m->N * D, w.qa_img, w.qkv_b, ws.x + (size_t)Bn * L * D, w.ln1_g, w.ln1_b,
                                                (bf16_t*)ao + (size_t)Bn * L * D, Bi, L, m->H, D, m->extras, s));
            }
            return DD_OK;
        }
        if (!in.qkv) {
            GemmArgs<T> g{h, nullptr, (const T*)w.qkv_w, w.qkv_b, nullptr, qkv, M, 3 * D, D, D, D, 0, 3 * D};
            g.hm = make_head_major(L, m->H);     // head-major: each (q | k | v, head) unit of an image is contiguous (attention.hip)
            DD_HIP(c, launch_gemm<T>(g, w.qkv_b ? EPI_BIAS_STORE : EPI_STORE, s, ch.cus));
        }
        // (the kernel is a function of the model, never of the call: beyond 288 tokens K / V stream through LDS; such a model is never perturbed
        // -- check_perturbed -- so the identity launch below keeps launch_v_copy's bound)
        if (Bn > 0) DD_TIMED(DD_PROF_QKV_ATTENTION, L > 288 ? launch_attention_long<T>(qkv, ao, Bn, L, m->H, D, s) : launch_attention<T>(qkv, ao, Bn, L, m->H, D, s));
        if (Bi > 0)
            DD_HIP(c, launch_v_copy<T>(qkv + (size_t)Bn * 3 * D * make_head_major(L, m->H).Lp, ao + (size_t)Bn * L * D, Bi, L, m->H, D, s));
        return DD_OK;
    }

    // x += attn.proj(ao) + b, then norm2 into h -- both in the fused block tail where the model has it (fused_proj; fused_mlp: norm2)
    int proj(int bi) {
        const BlockW& w = m->blocks[bi];
        GemmArgs<T> g{ao, nullptr, (const T*)w.proj_w, w.proj_b, ws.x, nullptr, M, D, D, D, D, 0, D};
        g.tile128 = tile128(D, D, D);
        if constexpr (bf16) {
            if (m->rowlin_proj) return rowlin_then_reduce(g, 1, w.rlp_img, w.ln2_g, w.ln2_b, false);
            if (m->splitk) return splitk_then_reduce_ln(g, 1, w.ln2_g, w.ln2_b, false);
            if (m->fused_proj) return DD_OK;
        }
        DD_HIP(c, launch_gemm<T>(g, EPI_BIAS_RESID, s, ch.cus));
        if (!(bf16 && m->fused_mlp)) DD_HIP(c, launch_layernorm<T>(ws.x, w.ln2_g, w.ln2_b, h, M, D, s));   // fused MLP: norm2 in its prologue
        return DD_OK;
    }

    // x += mlp.fc2(gelu(mlp.fc1(norm2))) + b and the T-typed copy of the block output, which feeds a later skip_linear: as the `skip` operand
    // (in-blocks) or as the `x` operand (mid / out blocks, except the last).  Leaves `next`: what the next block finds done.
    int mlp(int bi, Handoff& next) {
        const BlockW& w = m->blocks[bi];
        const bool is_in = bi < m->half_depth;   // the next block starts with norm1 (no skip_linear in between)
        const BlockW* wn = bi + 1 < nb ? &m->blocks[bi + 1] : nullptr;
        T* copy = is_in ? (T*)ws.skips[bi] : bi == deep_last ? (T*)bc.last : (wn ? xb : nullptr);
        const bool ln_next = is_in && !ends_outer(bi);   // the row passes below write that norm1 -- not for a block that will not run
        const Handoff in = next;     // (what this block found: the residual rows' form is this stage's to read)
        next = Handoff{};
        if constexpr (bf16) {
            if (m->fused_mlp) return block_tail(bi, copy, in, next);
        }
        GemmArgs<T> g1{h, nullptr, (const T*)w.fc1_w, w.fc1_b, nullptr, hid, M, m->hidden, D, D, D, 0, m->hid_ld};
        g1.tile128 = tile128(m->hidden, D, D);
        DD_TIMED(DD_PROF_FC1, launch_gemm<T>(g1, EPI_BIAS_GELU, s, ch.cus));
        GemmArgs<T> g{hid, nullptr, (const T*)w.fc2_w, w.fc2_b, ws.x, copy, M, D, m->hidden, m->hidden, m->hid_ld, m->hid_ld, D};
        g.tile128 = tile128(D, m->hidden, m->hidden);
        if constexpr (bf16) {   // (the row passes write the next block's norm1 where it starts with one)
            const float *ln_g = ln_next ? wn->ln1_g : nullptr, *ln_b = ln_next ? wn->ln1_b : nullptr;
            if (ln_next && (m->rowlin_fc2 || m->splitk)) next = norm1_written();
            if (m->rowlin_fc2) return rowlin_then_reduce(g, 1, w.rl_img, ln_g, ln_b, m->fused_qa);
            if (m->splitk) return splitk_then_reduce_ln(g, 1, ln_g, ln_b, m->fused_qa);
        }
        DD_HIP(c, launch_gemm<T>(g, EPI_BIAS_RESID, s, ch.cus));
        return DD_OK;
    }

    // (bf16) the fused block tail: [attn.proj +] norm2 + the MLP in one launch (mlp_fused.hip), with whatever the next block starts with
    // behind it -- its norm1; its skip_linear first (fused_skip); its attn.qkv last (fused_qkv), unless its attention launch computes that (fused_qa)
    int block_tail(int bi, T* copy, const Handoff in, Handoff& next) {
        const BlockW& w = m->blocks[bi];
        MlpFusedArgs fa{};
        fa.wimg = w.mlp_img; fa.b1p = w.mlp_b1p; fa.b2 = w.fc2_b;
        fa.ln_in_g = w.ln2_g; fa.ln_in_b = w.ln2_b;                       // norm2 of this block, in the prologue
        fa.xres = ws.x; fa.out = (bf16_t*)copy; fa.partial = ws.mlp_partial;
        if (m->fused_proj) { fa.ao = (const bf16_t*)ao; fa.bproj = w.proj_b; }
        if (ao_in_frag) fa.ao_frag = ws.aofrag;
        // the long-skip operand's patch rows: in-block bi's copy into its fragment buffer, read back by the tail that runs out-block nb - 1 - bi's skip_linear
        // (not in-block K - 1's under block caching: out-block nb - K reads them row-major)
        if (m->frag_skip && bi < m->half_depth && bi + 1 != deep_first) fa.out_frag = ws.skipfrags[bi];
        next.skip = m->fused_skip && bi >= m->half_depth && bi + 1 < nb && bi != deep_last;   // the next block starts with skip_linear
        if (next.skip) {
            fa.skip = (const bf16_t*)skip_of(bi + 1);
            if (m->frag_skip) fa.skip_frag = ws.skipfrags[nb - 1 - (bi + 1)];
            if (ee) fa.y_tap = ws.ytap;                                       // the next block's head / probe read y, which this launch consumes
            fa.bskip = m->blocks[bi + 1].skip_b;
        }
        // the next block's norm1 where it starts with one (behind its skip_linear, if this launch runs that); its attn.qkv inside its attention
        // launch (fused_qa), else last of all in this launch (fused_qkv) -- wherever this launch leaves that block's norm1
        const bool h_next = (bi < m->half_depth || next.skip) && !ends_outer(bi);
        // the residual patch rows: from xfrag where the previous tail left them there, into xfrag where the next launch to touch them is another tail
        // (h_next: no skip_linear launch in between); the last tail writes x for the output head -- fragment order lives between tails only
        if (in.xfrag) fa.x_in_frag = ws.xfrag;
        next.xfrag = m->frag_x && h_next;
        if (next.xfrag) fa.x_out_frag = ws.xfrag;
        next.frag = m->fused_qa && h_next;
        next.qkv = !next.frag && m->fused_qkv && h_next;
        next.h = h_next && !next.frag && !next.qkv;
        if (h_next) { fa.ln_out_g = m->blocks[bi + 1].ln1_g; fa.ln_out_b = m->blocks[bi + 1].ln1_b; fa.ln_out = (bf16_t*)h; }
        if (next.frag) fa.ln_out_frag = ws.hfrag;      // the patch rows' norm1 in the order the attention launch loads it
        if (next.qkv) { fa.qkv_out = (bf16_t*)qkv; fa.qkv_dump = ws.qkv_dump; }   // (norm1: the extra-token rows only)
        block_tail_plan(fa, B, m->N, m->extras, D, m->H, m->hidden, bi + 1 == nb);
        DD_TIMED(DD_PROF_BLOCK_TAIL, launch_mlp_fused(fa, D, s));   // (the event pair brackets the fused kernel alone)
        DD_HIP(c, block_tail_finish(fa, D, s));
        return DD_OK;
    }

    // block caching, in front of the seam's skip_linear.  A refresh: nothing (cache_rotate has run in front of the forward).  A reuse that
    // extrapolates: y^ = last + w (last - prev) into yhat, by the table's row or by cu.w.
    int cache_seam() {
        if (!cu.reuse || !cu.extrapolate) return DD_OK;
        DD_HIP(c, launch_cache_extrapolate(bc.last, bc.prev, bc.yhat, (long long)M * D, bf16, ch.st, cu.atab, CACHE_EXTRAPOLATE, cu.w, s));
        return DD_OK;
    }
    // prev <- last, in front of a refresh that rotates
    int cache_rotate() {
        if (!cu.blocks || cu.reuse || !cu.rotate) return DD_OK;
        DD_HIP(c, hipMemcpyAsync(bc.prev, bc.last, (size_t)M * D * sizeof(T), hipMemcpyDeviceToDevice, s));
        return DD_OK;
    }

    // every layer's unpatchify + conv in one launch (layer i: images [i B, (i + 1) B) of nb B, its own conv weights), every MLP probe's mean in one
    int ee_finish() {
        if (!ee_dec_all || B_full) return DD_OK;
        FinalArgs fa = final_args(m, ch, ee_dec_all, m->heads[0].wconv, m->heads[0].bconv, nb * B);
        fa.eps_out = ee->outs;
        fa.layer_B = B; fa.w_stride = m->ee_wconv_stride; fa.b_stride = m->ee_bconv_stride;
        DD_HIP(c, launch_final(fa, s));
        if (m->ee_type != DD_EE_ATTENTION_PROBE) DD_HIP(c, launch_ee_probe_reduce(ee_srow_all, ee->cls, nb * B, L, s));
        return DD_OK;
    }

    // output head (uvit.py:377-378): final LayerNorm in fp32 into scratch (the MLP hidden buffer is
    // free here), then decoder_pred as an exact-fp32 MFMA GEMM in BOTH precision modes, so eps is
    // never rounded to bf16.  dec holds all L tokens per image; the extras are skipped downstream.
    int head() {
        const HeadW& hd = m->head;
        if (hd.wg) {   // fused: rows read once, normalised rows never written
            HeadDecArgs ha{ws.x, hd.wg, hd.dc, ws.dec, M, m->pd, (L - m->extras) % 16 == 0 ? L : 0, m->extras};   // (only the patch rows)
            DD_HIP(c, launch_head_dec(ha, D, ch.cus, s));
            return DD_OK;
        }
        float* hf = (float*)ws.hid;
        DD_HIP(c, launch_layernorm<float>(ws.x, hd.ng, hd.nb, hf, M, D, s));
        GemmArgs<float> g{hf, nullptr, hd.wdec, hd.bdec, ws.dec, nullptr, M, m->pd, D, D, D, 0, m->pd};
        DD_HIP(c, launch_gemm<float>(g, EPI_BIAS_SET, s, ch.cus));
        return DD_OK;
    }
#undef DD_TIMED
};

template <typename T>
int run_backbone(dd_model* m, const Chain& ch, const float* x_img, const float* t_vec, const int64_t* y_dev, int B, hipStream_t s,
                 const EeTaps* ee = nullptr, Perturb pert = {}, const CacheUse& cu = {}) {
    Backbone<T> f{m, ch, B, s, ee, pert.first, pert.mask, cu};
    Handoff hand;
    if (int rc = f.cache_rotate()) return rc;
    if (int rc = f.embed(x_img, t_vec, y_dev, hand)) return rc;
    for (int bi = 0; bi < f.nb; ++bi) {
        if (bi == f.deep_first && cu.reuse) {      // the deep blocks do not run: on to the out-block behind them, which starts from y^ alone
            bi = f.deep_last + 1;
            hand = Handoff{};
            if (int rc = f.cache_seam()) return rc;
        }
        bool side = false;   // this block's early-exit head / probe launches are in flight on the side stream
        if (int rc = f.ee_taps(bi, hand, side)) return rc;
        if (int rc = f.skip_linear(bi, hand)) return rc;
        if (int rc = f.norm1_attention(bi, hand)) return rc;
        if (side) DD_HIP(m->ctx, hipStreamWaitEvent(s, m->ctx->ev_ee_join, 0));   // the head / probe launches have read x: from here on the block updates it
        if (int rc = f.proj(bi)) return rc;
        if (int rc = f.mlp(bi, hand)) return rc;
    }
    if (int rc = f.ee_finish()) return rc;
    return f.head();
}

int run_model(dd_model* m, const Chain& ch, const float* x_img, const float* t_vec, const int64_t* y_dev, int B, hipStream_t s,
              const EeTaps* ee = nullptr, Perturb pert = {}, const CacheUse& cu = {}) {
    return m->prec == DD_PREC_BF16 ? run_backbone<bf16_t>(m, ch, x_img, t_vec, y_dev, B, s, ee, pert, cu)
                                   : run_backbone<float>(m, ch, x_img, t_vec, y_dev, B, s, ee, pert, cu);
}

// run_backbone's stages one at a time, on the active prefix of a chain (dd_sample_early_exit_real)
template <typename T>
int real_stage(dd_model* m, const Chain& ch, const RealStage& r, Handoff& hand, hipStream_t s) {
    Backbone<T> f{m, ch, r.B, s, r.ee, 0, 0, CacheUse{}, r.B_full};
    switch (r.kind) {
    case REAL_EMBED:
        hand = Handoff{};
        return f.embed(r.x_img, nullptr, r.y, hand);
    case REAL_TAPS: {
        bool side = false;      // (the chain's Chain has ee_fork off: the decision behind the taps is in line with them)
        return f.ee_taps(r.bi, hand, side);
    }
    case REAL_BLOCK:
        if (int rc = f.skip_linear(r.bi, hand)) return rc;
        if (int rc = f.norm1_attention(r.bi, hand)) return rc;
        if (int rc = f.proj(r.bi)) return rc;
        return f.mlp(r.bi, hand);
    default: {
        if (int rc = f.head()) return rc;
        FinalArgs fa = final_args(m, ch, ch.ws->dec, m->head.wconv, m->head.bconv, r.B);
        fa.eps_out = r.eps;
        DD_HIP(m->ctx, launch_final(fa, s));
        return DD_OK;
    }
    }
}

// the checks of a call that do not concern labels
int check_model(dd_ctx* c, dd_model* m, int B) {
    if (!c || !m) return DD_ERR_INVALID;
    if (m->ctx != c) return ctx_fail(c, DD_ERR_INVALID, "model belongs to another context");
    if (!m->finalized) return ctx_fail(c, DD_ERR_STATE, "dd_model_finalize has not been called");
    if (B < 1 || B > m->cfg.max_batch) return ctx_fail(c, DD_ERR_INVALID, "batch size outside [1, max_batch]");
    return DD_OK;
}
}  // namespace

namespace dd {
int real_exit_stage(dd_model* m, const Chain& ch, const RealStage& r, Handoff& hand, hipStream_t s) {
    return m->prec == DD_PREC_BF16 ? real_stage<bf16_t>(m, ch, r, hand, s) : real_stage<float>(m, ch, r, hand, s);
}

int check_call(dd_ctx* c, dd_model* m, int B, const int64_t* y_dev) {
    if (int rc = check_model(c, m, B)) return rc;
    if (m->cfg.num_classes > 0 && !y_dev)
        return ctx_fail(c, DD_ERR_INVALID, "class-conditional model called without labels (pos_embed has L=extras+N rows)");
    if (m->cfg.num_classes <= 0 && y_dev)
        return ctx_fail(c, DD_ERR_INVALID, "unconditional model called with labels");
    return DD_OK;
}

// a guided call of B images on m (include/duodiff.h dd_guidance): every check before anything is enqueued
int check_guided(dd_ctx* c, dd_model* m, int B, const int64_t* y_dev, const dd_guidance* g) {
    if (!c || !m) return DD_ERR_INVALID;
    if (!g) return ctx_fail(c, DD_ERR_INVALID, "null dd_guidance");
    if (m->cfg.num_classes <= 0) return ctx_fail(c, DD_ERR_INVALID, "classifier-free guidance needs a class-conditional model");
    if (m->ee_type >= 0) return ctx_fail(c, DD_ERR_INVALID, "classifier-free guidance is not supported for early-exit models");
    if (g->null_label < 0 || g->null_label >= m->cfg.num_classes)
        return ctx_fail(c, DD_ERR_INVALID, "guidance null_label outside [0, num_classes) of the model");
    if (!std::isfinite(g->scale)) return ctx_fail(c, DD_ERR_INVALID, "guidance scale is not finite");
    if (B < 1 || 2LL * B > m->cfg.max_batch)
        return ctx_fail(c, DD_ERR_INVALID, "a guided batch of B images runs 2 B backbone rows: need 1 <= B and 2 B <= max_batch");
    return check_call(c, m, 2 * B, y_dev);
}

// a perturbed call of B images on m with the blocks of `mask` perturbed (include/duodiff.h dd_pag): every check before anything is enqueued
int check_perturbed(dd_ctx* c, dd_model* m, int B, const int64_t* y_dev, const dd_pag* p, unsigned mask) {
    if (!c || !m) return DD_ERR_INVALID;
    if (!p) return ctx_fail(c, DD_ERR_INVALID, "null dd_pag");
    if (!std::isfinite(p->scale)) return ctx_fail(c, DD_ERR_INVALID, "perturbed-attention guidance scale is not finite");
    if (m->cfg.depth < 32 && (mask >> m->cfg.depth)) return ctx_fail(c, DD_ERR_INVALID, "perturbed-attention mask names a block at or above the depth of the model");
    if (B < 1 || 2LL * B > m->cfg.max_batch)
        return ctx_fail(c, DD_ERR_INVALID, "a perturbed batch of B images runs 2 B backbone rows: need 1 <= B and 2 B <= max_batch");
    if (m->ee_type >= 0) return ctx_fail(c, DD_ERR_INVALID, "perturbed-attention guidance is not supported for early-exit models");
    if (m->L > 288) return ctx_fail(c, DD_ERR_UNSUPPORTED, "perturbed-attention guidance: sequence length must be <= 288 tokens (the identity launches)");
    return check_call(c, m, 2 * B, y_dev);
}

// block caching with K = blocks on m (include/duodiff.h dd_block_cache): a plain model, 1 <= K <= depth / 2
int check_cached(dd_ctx* c, dd_model* m, int blocks) {
    if (!c || !m) return DD_ERR_INVALID;
    if (m->ee_type >= 0) return ctx_fail(c, DD_ERR_INVALID, "block caching is not supported for early-exit models");
    if (blocks < 1 || blocks > m->half_depth)
        return ctx_fail(c, DD_ERR_INVALID, "block caching: blocks = " + std::to_string(blocks) + " outside [1, depth / 2 = " + std::to_string(m->half_depth) + "] of the model");
    return DD_OK;
}

// an autoguided call of B images (include/duodiff.h dd_autoguidance) on first (and late, or null): every check before anything is enqueued
int check_autoguided(dd_ctx* c, dd_model* first, dd_model* late, int B, const int64_t* y_dev, const dd_autoguidance* ag) {
    if (!c || !first) return DD_ERR_INVALID;
    if (!ag) return ctx_fail(c, DD_ERR_INVALID, "null dd_autoguidance");
    dd_model* gm = ag->guide;
    if (!gm) return ctx_fail(c, DD_ERR_INVALID, "null guide model");
    if (gm->ctx != c) return ctx_fail(c, DD_ERR_INVALID, "guide model belongs to another context");
    if (gm->ee_type >= 0) return ctx_fail(c, DD_ERR_INVALID, "autoguidance is not supported for early-exit models (the guide carries heads)");
    if (!gm->finalized) return ctx_fail(c, DD_ERR_INVALID, "guide model: dd_model_finalize has not been called");
    if (!std::isfinite(ag->scale)) return ctx_fail(c, DD_ERR_INVALID, "autoguidance scale is not finite");
    bool conditional = gm->cfg.num_classes > 0;
    for (dd_model* m : {first, late}) {
        if (!m) continue;
        if (m->ctx == c && m->ee_type >= 0) return ctx_fail(c, DD_ERR_INVALID, "autoguidance is not supported for early-exit models");
        if (int rc = check_model(c, m, B)) return rc;
        if (m->cfg.img_size != gm->cfg.img_size || m->cfg.patch_size != gm->cfg.patch_size || m->cfg.in_chans != gm->cfg.in_chans)
            return ctx_fail(c, DD_ERR_INVALID, "guide model disagrees with the guided model on image geometry (img_size, patch_size, in_chans)");
        conditional = conditional || m->cfg.num_classes > 0;
    }
    if (B > gm->cfg.max_batch) return ctx_fail(c, DD_ERR_INVALID, "batch size outside [1, max_batch] of the guide model");
    if (conditional && !y_dev) return ctx_fail(c, DD_ERR_INVALID, "autoguidance with a class-conditional model called without labels");
    if (!conditional && y_dev) return ctx_fail(c, DD_ERR_INVALID, "autoguidance of unconditional models called with labels");
    return DD_OK;
}
}  // namespace dd

namespace {
// the guide's side of chain ch of model m: the same chain of the guide's own workspaces, the same step state and grids
Chain guide_chain(const Chain& ch, const dd_model* m, const dd_model* guide) {
    Chain g = ch;
    g.ws = &guide->ws[ch.ws == &m->ws[1] ? 1 : 0];
    return g;
}
// Under autoguidance the running model m is guided unless it is the guide model itself (the plain unguided step).  Runs the guide's
// forward in line on the chain's stream (no fork inside a captured step: parallel branches in a chain's graph cost more than they hide,
// and the other chain already fills the chip) and points the output head's second halo at its decoder rows.  Both embed launches copy
// the same t into the step state (rowops.hip: t_final = t); only the output head advances it.
int run_guide(dd_ctx* c, dd_model* m, const Chain& ch, const dd_autoguidance* ag, const float* x_dev, const int64_t* y_dev, int B,
              hipStream_t s, FinalArgs& fa) {
    dd_model* gm = ag->guide;
    const Chain gch = guide_chain(ch, m, gm);
    if (int rc = run_model(gm, gch, x_dev, nullptr, gm->cfg.num_classes > 0 ? y_dev : nullptr, B, s)) return rc;
    fa.dec2 = gch.ws->dec; fa.wconv2 = gm->head.wconv; fa.bconv2 = gm->head.bconv; fa.L2 = gm->L; fa.extras2 = gm->extras;
    fa.guide_scale = ag->scale;
    return DD_OK;
}

// eps = model(x, t) of B images of chain ch enqueued on s, up to the output head: the guide's forward (autoguidance; each model takes
// y_dev iff it is class-conditional), the model's (classifier-free guidance: 2 B rows in stage_guided's layout) and the head's arguments
// that combine them.  The caller sets what the head writes and launches it.
int model_eps(dd_ctx* c, dd_model* m, const Chain& ch, const float* x_dev, const int64_t* y_dev, int B, hipStream_t s, const StepOpts& o,
              FinalArgs& fa) {
    const dd_guidance* g = o.mods.g;
    const dd_autoguidance* ag = o.mods.ag;
    if (o.t_set) DD_HIP(c, launch_set_state_float(ch.st, *o.t_set, s));
    fa = final_args(m, ch, ch.ws->dec, m->head.wconv, m->head.bconv, B);
    int rc = DD_OK;
    if (ag && ag->guide != m && (rc = run_guide(c, m, ch, ag, x_dev, y_dev, B, s, fa))) return rc;
    if (ag && m->cfg.num_classes <= 0) y_dev = nullptr;
    const dd_pag* pag = o.mods.pag;
    const Perturb pert = pag ? Perturb{B, o.mods.pag_mask(m)} : Perturb{};
    if ((rc = run_model(m, ch, x_dev, o.t_vec, y_dev, g || pag ? 2 * B : B, s, o.ee, pert, o.cache))) return rc;
    if (g) { fa.pair_B = B; fa.guide_scale = g->scale; }
    if (pag) { fa.pair_B = B; fa.guide_scale = pag->scale; }
    return DD_OK;
}
}  // namespace

namespace dd {
// one sampling step of chain ch enqueued on s: x <- update(x, model(x, t)); t comes from ch.st
int enqueue_step(dd_ctx* c, dd_model* m, const Chain& ch, float* x_dev, const int64_t* y_dev, int B, hipStream_t s, const StepOpts& o) {
    FinalArgs fa;
    if (int rc = model_eps(c, m, ch, x_dev, y_dev, B, s, o, fa)) return rc;
    if (o.thr) {   // the head writes the (guided) m and nothing else; the step's rule, its noise, the known region and the advance are the second launch's
        fa.eps_out = o.m_scratch; fa.atab = o.atab; fa.b0 = o.b0;
        DD_HIP(c, launch_final(fa, s));
        ThresholdArgs ta{x_dev, o.m_scratch, nullptr, o.h, x_dev};
        ta.st = ch.st; ta.coef = c->coef; ta.atab = o.atab; ta.htab = o.htab;
        ta.noise_mode = o.noise_mode; ta.advance = o.advance; ta.b0 = o.b0; ta.pair_B = fa.pair_B;
        ta.kx0 = o.mods.kn.x0; ta.kmask = o.mods.kn.mask; ta.ktab = o.mods.kn.ktab;
        ta.thr = *o.thr; ta.B = B; ta.C = m->cfg.in_chans; ta.S = m->cfg.img_size; ta.seeds = o.mods.seeds;
        DD_HIP(c, launch_threshold_step(ta, s));
        return DD_OK;
    }
    fa.x_in = x_dev; fa.z = o.z; fa.eps_out = o.eps_out; fa.x_out = x_dev;
    fa.noise_mode = o.noise_mode; fa.variance = o.variance; fa.advance = o.advance; fa.atab = o.atab; fa.b0 = o.b0;
    fa.htab = o.htab; fa.h = o.h;
    fa.kx0 = o.mods.kn.x0; fa.kmask = o.mods.kn.mask; fa.ktab = o.mods.kn.ktab;
    fa.seeds = o.mods.seeds;
    DD_HIP(c, launch_final(fa, s));
    return DD_OK;
}

int check_image_seeds(dd_ctx* c, int noise_mode, int B) {
    if (c->seeds_user && noise_mode == DD_NOISE_PHILOX && c->seeds_n != B)
        return ctx_fail(c, DD_ERR_INVALID, "dd_set_image_seeds holds " + std::to_string(c->seeds_n) + " seeds, the call has " + std::to_string(B) + " images");
    return DD_OK;
}
int stage_image_seeds(dd_ctx* c, int noise_mode, hipStream_t s, const unsigned long long** seeds) {
    *seeds = nullptr;
    if (!c->seeds_user || noise_mode != DD_NOISE_PHILOX) return DD_OK;
    if (int rc = c->seeds_stage.grow(c, (size_t)c->seeds_n)) return rc;
    DD_HIP(c, hipMemcpyAsync(c->seeds_stage.p, c->seeds_user, (size_t)c->seeds_n * sizeof(unsigned long long), hipMemcpyDeviceToDevice, s));
    *seeds = c->seeds_stage.p;
    return DD_OK;
}

// eps = model(x, t) and nothing else (dd_forward*, the early-exit step): the step-only options are not read
int forward_eps(dd_ctx* c, dd_model* m, const Chain& ch, const float* x_dev, const int64_t* y_dev, float* eps_dev, int B, hipStream_t s,
                const StepOpts& o) {
    FinalArgs fa;
    if (int rc = model_eps(c, m, ch, x_dev, y_dev, B, s, o, fa)) return rc;
    fa.eps_out = eps_dev;
    DD_HIP(c, launch_final(fa, s));
    return DD_OK;
}
}  // namespace dd

namespace {
// dd_sample / dd_sample_affine with graphs: the loop runs on context-owned staging copies of x / y, so the captured step
// does not depend on the caller's tensor addresses
int grow_stage(dd_ctx* c, size_t x_elems, size_t y_elems) {
    if (int rc = c->x_stage.grow(c, x_elems)) return rc;
    return c->y_stage.grow(c, y_elems);
}
}  // namespace

namespace dd {
int stage_inputs(dd_ctx* c, const float* x_dev, const int64_t* y_dev, int B, size_t x_elems, hipStream_t s, float** x_run,
                 const int64_t** y_run) {
    if (int rc = grow_stage(c, x_elems, y_dev ? (size_t)B : 0)) return rc;
    DD_HIP(c, hipMemcpyAsync(c->x_stage.p, x_dev, x_elems * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (y_dev) DD_HIP(c, hipMemcpyAsync(c->y_stage.p, y_dev, (size_t)B * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    *x_run = c->x_stage.p;
    *y_run = y_dev ? c->y_stage.p : nullptr;
    return DD_OK;
}

// A guided call (eager or graph-replayed) always runs on the staging buffers, 2 B images: chain k (images [o_k, o_k + B_k), o_0 = 0,
// o_1 = B0) owns images [2 o_k, 2 o_k + 2 B_k) of them -- its B_k images, then the same images again -- and labels [y_k | null x B_k];
// null_label < 0 (perturbed-attention guidance): the second half's labels are the first half's, [y_k | y_k], or none (y_dev null).
// B0 == B: one chain.
int stage_guided(dd_ctx* c, const float* x_dev, const int64_t* y_dev, int B, int B0, size_t chw, int null_label, hipStream_t s,
                 float** x_run, const int64_t** y_run) {
    if (int rc = grow_stage(c, 2 * (size_t)B * chw, y_dev ? 2 * (size_t)B : 0)) return rc;
    for (int k = 0; k < 2; ++k) {
        const int o = k ? B0 : 0, Bk = k ? B - B0 : B0;
        if (Bk == 0) continue;
        float* xs = c->x_stage.p + 2 * (size_t)o * chw;
        DD_HIP(c, hipMemcpyAsync(xs, x_dev + (size_t)o * chw, (size_t)Bk * chw * sizeof(float), hipMemcpyDeviceToDevice, s));
        DD_HIP(c, hipMemcpyAsync(xs + (size_t)Bk * chw, x_dev + (size_t)o * chw, (size_t)Bk * chw * sizeof(float), hipMemcpyDeviceToDevice, s));
        if (null_label >= 0) {
            DD_HIP(c, launch_guided_labels((const long long*)y_dev + o, (long long*)c->y_stage.p + 2 * (size_t)o, Bk, null_label, s));
        } else if (y_dev) {
            for (int half = 0; half < 2; ++half)
                DD_HIP(c, hipMemcpyAsync(c->y_stage.p + 2 * (size_t)o + (size_t)half * Bk, y_dev + o, (size_t)Bk * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
        }
    }
    *x_run = c->x_stage.p;
    *y_run = y_dev ? c->y_stage.p : nullptr;
    return DD_OK;
}
// ... and the first half of each chain's block back to the caller's images
int unstage_guided(dd_ctx* c, float* x_dev, const float* x_run, int B, int B0, size_t chw, hipStream_t s) {
    for (int k = 0; k < 2; ++k) {
        const int o = k ? B0 : 0, Bk = k ? B - B0 : B0;
        if (Bk) DD_HIP(c, hipMemcpyAsync(x_dev + (size_t)o * chw, x_run + 2 * (size_t)o * chw, (size_t)Bk * chw * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    return DD_OK;
}
}  // namespace dd

// ==========================================================================================
extern "C" {

int dd_forward(dd_ctx* c, dd_model* m, const float* x_dev, float t, const float* t_dev, const int64_t* y_dev,
               float* eps_dev, int B, void* stream) {
    int rc = check_call(c, m, B, y_dev);
    if (rc) return rc;
    if (!x_dev || !eps_dev) return ctx_fail(c, DD_ERR_INVALID, "null tensor");
    return forward_eps(c, m, whole_batch(c, m), x_dev, y_dev, eps_dev, B, (hipStream_t)stream, {.t_set = &t, .t_vec = t_dev});
}

int dd_forward_early_exit(dd_ctx* c, dd_model* m, const float* x_dev, float t, const float* t_dev, const int64_t* y_dev,
                          float* eps_dev, float* classifier_dev, float* outputs_dev, int B, void* stream) {
    int rc = check_call(c, m, B, y_dev);
    if (rc) return rc;
    if (m->ee_type < 0) return ctx_fail(c, DD_ERR_STATE, "model was not created with dd_model_enable_early_exit");
    if (!x_dev || !eps_dev || !classifier_dev || !outputs_dev) return ctx_fail(c, DD_ERR_INVALID, "null tensor");
    const int ti = (int)t;                                   // t = int(timesteps[0]) (early_exit.py:271)
    if (m->ee_type != DD_EE_MLP_PER_LAYER && m->ee_type != DD_EE_ATTENTION_PROBE && (ti < 0 || ti > 999)) return ctx_fail(c, DD_ERR_NOT_FOUND, "no probe for this timestep (KeyError in the reference)");
    const EeTaps ee{classifier_dev, outputs_dev, ti};
    return forward_eps(c, m, whole_batch(c, m), x_dev, y_dev, eps_dev, B, (hipStream_t)stream, {.t_set = &t, .t_vec = t_dev, .ee = &ee});
}

int dd_forward_guided(dd_ctx* c, dd_model* m, const float* x_dev, float t, const int64_t* y_dev, const dd_guidance* g,
                      float* eps_dev, int B, void* stream) {
    int rc = check_guided(c, m, B, y_dev, g);
    if (rc) return rc;
    if (!x_dev || !eps_dev) return ctx_fail(c, DD_ERR_INVALID, "null tensor");
    hipStream_t s = (hipStream_t)stream;
    const size_t chw = (size_t)m->cfg.in_chans * m->cfg.img_size * m->cfg.img_size;
    float* x_run = nullptr;
    const int64_t* y_run = nullptr;
    if ((rc = stage_guided(c, x_dev, y_dev, B, B, chw, g->null_label, s, &x_run, &y_run))) return rc;
    return forward_eps(c, m, whole_batch(c, m), x_run, y_run, eps_dev, B, s, {.t_set = &t, .mods = {.g = g}});
}

int dd_forward_cached(dd_ctx* c, dd_model* m, const float* x_dev, float t, const int64_t* y_dev, const dd_guidance* g, int blocks, int op,
                      float w, float* eps_dev, int B, void* stream) {
    if (c && m && m->ctx == c && m->ee_type >= 0) return ctx_fail(c, DD_ERR_INVALID, "block caching is not supported for early-exit models");
    int rc = g ? check_guided(c, m, B, y_dev, g) : check_call(c, m, B, y_dev);
    if (rc || (rc = check_cached(c, m, blocks))) return rc;
    if (!x_dev || !eps_dev) return ctx_fail(c, DD_ERR_INVALID, "null tensor");
    if (op < CACHE_REFRESH || op > CACHE_EXTRAPOLATE) return ctx_fail(c, DD_ERR_INVALID, "block caching: op outside {0, 1, 2}");
    if (op == CACHE_EXTRAPOLATE && !std::isfinite(w)) return ctx_fail(c, DD_ERR_INVALID, "block caching: the extrapolation weight is not finite");
    // the whole-batch chain's cache: a refresh always rotates (prev is then the refresh before the last one wherever two have run)
    BlockCache& bc = m->cache[0];
    const int rows = g ? 2 * B : B;
    if (op != CACHE_REFRESH && !bc.holds(blocks, rows, 0, B))
        return ctx_fail(c, DD_ERR_INVALID, "block caching: a reuse step, and the model holds no refresh of this batch and these blocks");
    if (op == CACHE_EXTRAPOLATE && !bc.has_prev)
        return ctx_fail(c, DD_ERR_INVALID, "block caching: an extrapolating reuse step, and the model holds no second refresh of this batch and these blocks");
    hipStream_t s = (hipStream_t)stream;
    if ((rc = ensure_block_cache(c, m, 0, s))) return rc;
    const float* x_run = x_dev;
    const int64_t* y_run = y_dev;
    if (g) {
        const size_t chw = (size_t)m->cfg.in_chans * m->cfg.img_size * m->cfg.img_size;
        float* xs = nullptr;
        if ((rc = stage_guided(c, x_dev, y_dev, B, B, chw, g->null_label, s, &xs, &y_run))) return rc;
        x_run = xs;
    }
    const CacheUse cu{blocks, op != CACHE_REFRESH, op == CACHE_REFRESH, op == CACHE_EXTRAPOLATE, w, nullptr};
    rc = forward_eps(c, m, whole_batch(c, m), x_run, y_run, eps_dev, B, s, {.t_set = &t, .mods = {.g = g}, .cache = cu});
    // the refresh counts once its forward is enqueued whole; one that failed on the way may have rotated or half-written the buffers: they hold nothing
    if (op == CACHE_REFRESH) {
        if (rc) bc.has_last = bc.has_prev = false;
        else bc.refresh(blocks, rows, 0, B, true);
    }
    return rc;
}

int dd_forward_autoguided(dd_ctx* c, dd_model* m, const float* x_dev, float t, const int64_t* y_dev, const dd_autoguidance* g,
                          float* eps_dev, int B, void* stream) {
    int rc = check_autoguided(c, m, nullptr, B, y_dev, g);
    if (rc) return rc;
    if (!x_dev || !eps_dev) return ctx_fail(c, DD_ERR_INVALID, "null tensor");
    return forward_eps(c, m, whole_batch(c, m), x_dev, y_dev, eps_dev, B, (hipStream_t)stream, {.t_set = &t, .mods = {.ag = g}});
}

int dd_forward_perturbed(dd_ctx* c, dd_model* m, const float* x_dev, float t, const int64_t* y_dev, const dd_pag* p, float* eps_dev, int B,
                         void* stream) {
    int rc = check_perturbed(c, m, B, y_dev, p, p ? p->layers_first : 0);
    if (rc) return rc;
    if (!x_dev || !eps_dev) return ctx_fail(c, DD_ERR_INVALID, "null tensor");
    hipStream_t s = (hipStream_t)stream;
    const size_t chw = (size_t)m->cfg.in_chans * m->cfg.img_size * m->cfg.img_size;
    float* x_run = nullptr;
    const int64_t* y_run = nullptr;
    if ((rc = stage_guided(c, x_dev, y_dev, B, B, chw, -1, s, &x_run, &y_run))) return rc;
    return forward_eps(c, m, whole_batch(c, m), x_run, y_run, eps_dev, B, s, {.t_set = &t, .mods = perturbed(p, nullptr)});
}

int dd_sample_step(dd_ctx* c, dd_model* m, float* x_dev, int t, const int64_t* y_dev, int noise_mode, const float* z_dev,
                   uint64_t seed, int variance, float* eps_out_dev, int B, void* stream) {
    int rc = check_call(c, m, B, y_dev);
    if (rc) return rc;
    if (!x_dev) return ctx_fail(c, DD_ERR_INVALID, "null tensor");
    if (t < 0 || t > 999) return ctx_fail(c, DD_ERR_INVALID, "timestep outside [0, 999]");
    if (noise_mode == DD_NOISE_BUFFER && !z_dev && t > 0) return ctx_fail(c, DD_ERR_INVALID, "DD_NOISE_BUFFER needs z_dev");
    if ((rc = check_image_seeds(c, noise_mode, B))) return rc;
    hipStream_t s = (hipStream_t)stream;
    const unsigned long long* seeds = nullptr;
    if ((rc = stage_image_seeds(c, noise_mode, s, &seeds))) return rc;
    DD_HIP(c, launch_set_state(c->st[0], t, (unsigned long long)seed, s));
    return enqueue_step(c, m, whole_batch(c, m), x_dev, y_dev, B, s,
                        {.mods = {.seeds = seeds}, .noise_mode = noise_mode, .z = z_dev, .variance = variance, .eps_out = eps_out_dev});
}

}  // extern "C"
