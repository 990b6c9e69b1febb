// The model behind a dd_model handle (include/duodiff.h), up to the point where it can run: the schedule constants, the catalogue of its
// state_dict, the kernel path of each stage, every weight packed into one arena and the activation workspace of each half-batch chain.
// The lowest of the four host units (engine_state.h): it calls no other, and defines ctx_fail, which all of them call.
//
// Host-side restatement of: UViT.__init__ (reference models/uvit.py:228-336), the early-exit heads and probes (models/early_exit.py:40-80,
// 193-268), schedule constants (sampler.py:40-44, ddpm_core.py:64-70).
#include "../../include/duodiff.h"
#include "../../include/duodiff_dev.h"
#include "engine_state.h"
#include "host_arena.h"
#include "launch_args.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <vector>

using namespace dd;

namespace dd {
// declared in dev_scope.h: every host unit reports its errors through it
int ctx_fail(dd_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}
}  // namespace dd

namespace {

// ---- schedule: bit-for-bit the fp32 tables of sampler.py:40-44 / ddpm_core.py:64-70 (see oracle/schedule_oracle.py)
// betas = torch.linspace(beta_init, beta_final, n): ATen rounds once per element, forward from start in the first half,
// backward from end in the second; alphas_bar = torch.cumprod: the CPU scan accumulates in double, rounds each output.
void base_tables(float beta_init, float beta_final, int n, float* betas, float* alphas, float* abar, float* abar_prev) {
    const float start = beta_init, end = beta_final;
    const float stepf = n > 1 ? (end - start) / (float)(n - 1) : 0.0f;
    const double step = (double)stepf;
    const int half = n / 2;
    for (int i = 0; i < n; ++i) {
        betas[i] = i < half ? (float)((double)start + step * i) : (float)((double)end - step * (n - 1 - i));
        alphas[i] = 1.0f - betas[i];
    }
    double run = 1.0;
    for (int i = 0; i < n; ++i) {
        run *= (double)alphas[i];
        abar[i] = (float)run;
    }
    for (int i = 0; i < n; ++i) abar_prev[i] = i ? abar[i - 1] : 1.0f;
}
float bt_sampler_order(float beta, float abar_prev, float abar) {   // sampler.py:44: betas * (1 - abar_prev) / (1 - abar)
    volatile float num = beta * (1.0f - abar_prev);
    return num / (1.0f - abar);
}
float bt_scheduler_order(float beta, float abar_prev, float abar) {   // ddpm_core.py:68-70: (1 - abar_prev) / (1 - abar) * betas
    volatile float ratio = (1.0f - abar_prev) / (1.0f - abar);
    return ratio * beta;
}

}  // namespace

namespace dd {
Schedule::Schedule() {
    base_tables(1e-4f, 0.02f, 1000, betas, alphas, abar, abar_prev);
    for (int i = 0; i < 1000; ++i) {
        bt_sampler[i] = bt_sampler_order(betas[i], abar_prev[i], abar[i]);
        bt_sched[i] = bt_scheduler_order(betas[i], abar_prev[i], abar[i]);
        c1[i] = sqrtf(1.0f / alphas[i]);
        c2[i] = (1.0f - alphas[i]) / sqrtf(1.0f - abar[i]);
        sigma[i] = sqrtf(bt_sampler[i]);
        sigma_beta[i] = sqrtf(betas[i]);
    }
}
const Schedule& schedule() {
    static const Schedule s;
    return s;
}
}  // namespace dd

namespace {

// the probes of an early-exit model (EarlyExitUViT.matrix, early_exit.py:194-204, 219-240) form an nt x nl grid of (timestep, layer);
// row t nl + layer of the probe table is probe (layer, t): per layer `layer`, per timestep `t`, per layer and timestep `t depth + layer`
void probe_grid(const dd_model* m, int& nt, int& nl) {
    nt = m->ee_type == DD_EE_MLP_PER_LAYER || m->ee_type == DD_EE_ATTENTION_PROBE ? 1 : 1000;
    nl = m->ee_type == DD_EE_MLP_PER_TIMESTEP ? 1 : m->cfg.depth;
}
std::string probe_key(const dd_model* m, int layer, int t) {
    switch (m->ee_type) {
        case DD_EE_MLP_PER_LAYER:
        case DD_EE_ATTENTION_PROBE: return std::to_string(layer);
        case DD_EE_MLP_PER_TIMESTEP: return std::to_string(t);
        default: return std::to_string(layer) + ", " + std::to_string(t);
    }
}
std::string block_prefix(const dd_model* m, int bi) {
    if (bi < m->half_depth) return "in_blocks." + std::to_string(bi) + ".";
    if (bi == m->half_depth) return "mid_block.";
    return "out_blocks." + std::to_string(bi - m->half_depth - 1) + ".";
}
std::string head_prefix(const dd_model* m, int layer) {
    if (layer < m->half_depth) return "in_blocks_heads." + std::to_string(layer) + ".";
    if (layer == m->half_depth) return "mid_block_head.";
    return "out_blocks_heads." + std::to_string(layer - m->half_depth - 1) + ".";
}

// every state_dict name of the model with its shape, nothing set (models/uvit.py:228-336; for ee_type >= 0 also the early-exit heads and
// probes, early_exit.py:40-80, 193-268): what dd_model_set_param accepts and dd_model_finalize requires
std::map<std::string, HostParam> catalogue(const dd_model* m) {
    std::map<std::string, HostParam> c;
    const int64_t D = m->D, C = m->cfg.in_chans, P = m->cfg.patch_size, hid = m->hidden;
    auto add = [&](const std::string& n, std::vector<int64_t> shape) { c[n].shape = std::move(shape); };
    auto linear = [&](const std::string& n, int64_t out, int64_t in) { add(n + ".weight", {out, in}); add(n + ".bias", {out}); };
    auto head = [&](const std::string& p) {
        add(p + "norm.weight", {D}); add(p + "norm.bias", {D});
        linear(p + "decoder_pred", m->pd, D);
        add(p + "final_layer.weight", {C, C, 3, 3}); add(p + "final_layer.bias", {C});
    };
    add("pos_embed", {1, m->L, D});
    add("patch_embed.proj.weight", {D, C, P, P}); add("patch_embed.proj.bias", {D});
    if (m->cfg.mlp_time_embed) { linear("time_embed.0", 4 * D, D); linear("time_embed.2", D, 4 * D); }
    if (m->cfg.num_classes > 0) add("label_emb.weight", {m->cfg.num_classes, D});
    for (int bi = 0; bi < m->cfg.depth; ++bi) {
        const std::string p = block_prefix(m, bi);
        add(p + "norm1.weight", {D}); add(p + "norm1.bias", {D});
        add(p + "attn.qkv.weight", {3 * D, D});
        if (m->cfg.qkv_bias) add(p + "attn.qkv.bias", {3 * D});
        linear(p + "attn.proj", D, D);
        add(p + "norm2.weight", {D}); add(p + "norm2.bias", {D});
        linear(p + "mlp.fc1", hid, D); linear(p + "mlp.fc2", D, hid);
        if (bi > m->half_depth) linear(p + "skip_linear", D, 2 * D);
    }
    head("");
    if (m->ee_type < 0) return c;
    for (int layer = 0; layer < m->cfg.depth; ++layer) head(head_prefix(m, layer));
    int nt, nl;
    probe_grid(m, nt, nl);
    for (int t = 0; t < nt; ++t)
        for (int layer = 0; layer < nl; ++layer) {
            const std::string p = "matrix." + probe_key(m, layer, t) + ".";
            if (m->ee_type == DD_EE_ATTENTION_PROBE) {
                add(p + "q", {1, 1, 1, D});
                linear(p + "weight_kv", 2 * D, D); linear(p + "classification.0", D, D); linear(p + "classification.2", 1, D);
            } else {
                linear(p + "classifier.0", 1, D);
            }
        }
    return c;
}

// Layout of one chain's activation workspace for batches up to `batch` (the model's max_batch; half of it, rounded up, for the second
// half-batch chain of dd_sample, which never runs more): the buffers of w as regions of a
void ws_layout(const dd_model* m, int batch, WsPtrs& w, Arena& a) {
    const int D = m->D, L = m->L, hid = m->hidden;
    const size_t es = m->esize;
    const size_t Mp = (size_t)round_up(batch * L, 256);
    // qkv is head-major: B * 3H units of Lp rows x 64 (rows [L, Lp) of a unit are never written: the bf16 attention launch that stages K / V
    // from this tensor zeroes them in its LDS images itself)
    const size_t qkv_elems = (size_t)batch * 3 * D * (size_t)make_head_major(L, m->H).Lp;
    a.space(w.x, Mp * D * 4); a.space(w.h, Mp * D * es); a.space(w.ao, Mp * D * es); a.space(w.qkv, std::max(Mp * 3 * D, qkv_elems) * es);
    a.space(w.hid, Mp * (size_t)m->hid_ld * es); a.space(w.xb, Mp * D * es);
    w.skips.assign(m->half_depth, nullptr);
    for (void*& sk : w.skips) a.space(sk, Mp * D * es);
    a.space(w.dec, Mp * m->pd * 4);
    const size_t part_bytes = m->fused_mlp ? mlp_fused_partial_bytes(batch, m->extras, D, hid)
                              : m->splitk ? (size_t)2 * Mp * D * 4
                              : m->rowlin_fc2 ? std::max(std::max(rowlin_partial_bytes(batch, m->extras, hid), rowlin_partial_bytes(batch, m->extras, 2 * D)), rowlin_partial_bytes(batch, m->extras, D)) : 0;
    if (part_bytes) a.space(w.mlp_partial, part_bytes);
    if (m->fused_qkv) a.space(w.qkv_dump, 16384);
    if (m->fused_qa) a.space(w.hfrag, (size_t)batch * m->N * D * 2);
    if (m->ee_type >= 0 && m->fused_skip) a.space(w.ytap, Mp * D * 4);
    const size_t patch_elems = (size_t)batch * m->N * D;
    if (m->frag_ao) a.space(w.aofrag, patch_elems * 2);
    w.skipfrags.assign(m->frag_skip ? m->half_depth : 0, nullptr);
    for (bf16_t*& sf : w.skipfrags) a.space(sf, patch_elems * 2);
    if (m->frag_x) a.space(w.xfrag, patch_elems * 4);
}
// ---- dd_model_finalize: the kernel path of each stage, then every weight packed into one arena
// (a function of the model, its precision and the development flags dd_dev_set_flags: never of a call's batch)
void choose_paths(dd_model* m, int precision, unsigned flags) {
    const int D = m->D, hid = m->hidden, L = m->L;
    // fused block tail (mlp_fused.hip): bf16 mode only (development A/B runs can switch it off: dd_dev_set_flags)
    m->fused_mlp = precision == DD_PREC_BF16 && mlp_fused_supported(D, hid) && !(flags & DD_DEV_NO_FUSED_MLP);
    m->fused_proj = m->fused_mlp && D % 128 == 0 && !(flags & DD_DEV_NO_FUSED_PROJ);
    m->fused_skip = m->fused_proj && (hid / 32) % 2 == 0 && !(flags & DD_DEV_NO_FUSED_SKIP);     // (early-exit models too: y leaves through MlpFusedArgs::y_tap)
    m->fused_qkv = m->fused_proj && m->ee_type < 0 && (hid / 32) % 2 == 0 && !m->cfg.qkv_bias && !(flags & DD_DEV_NO_FUSED_QKV);
    // (early-exit models too: their heads and probes read the residual stream between blocks, which this launch does not touch)
    // (embed_dim 768 / 1024 too, which have no fused block tail: their norm1 launch writes the fragment order, the qkv tensor is gone)
    m->fused_qa = precision == DD_PREC_BF16 && qkv_attention_supported(D, m->H, L, m->extras) && !(flags & DD_DEV_NO_FUSED_QA);
    // the patch rows' hand-offs in fragment order ride on that launch and the proj-fused tail (mlp_fused.hip FRAG: D = 512)
    const bool frag = m->fused_qa && m->fused_proj && D == 512 && m->N % 32 == 0;
    m->frag_ao = frag && !(flags & DD_DEV_NO_FRAG_AO);
    m->frag_skip = frag && m->fused_skip && !(flags & DD_DEV_NO_FRAG_SKIP);
    m->frag_x = frag && m->ee_type < 0 && !(flags & DD_DEV_NO_FRAG_X);
    // (embed_dim 768, no fused block tail) mlp.fc2 with the residual rows resident in registers: x read and written once, the next norm1 from registers
    m->rowlin_fc2 = precision == DD_PREC_BF16 && !m->fused_mlp && rowlin_supported(D, hid) && m->N % 32 == 0 && !(flags & DD_DEV_NO_ROWLIN);
    // (its operand row offsets are 32 bits: rows x hidden x 2 bytes < 2^32, 2427 images at 288 tokens.  A long-sequence model whose max_batch
    // passes that takes the GEMM sequence for every batch; the models of up to 288 tokens keep the launch's own check)
    if (L > 288 && (long long)m->cfg.max_batch * L * hid * 2 >= (1ll << 32)) m->rowlin_fc2 = false;
    m->rowlin_proj = m->rowlin_fc2 && !(flags & DD_DEV_NO_ROWLIN_PROJ);
    m->rowlin_skip = m->rowlin_fc2 && rowlin_supported(D, 2 * D) && !(flags & DD_DEV_NO_ROWLIN_SKIP);
    // split-K for the N = embed_dim Linears (skip_linear, attn.proj, mlp.fc2) where even max_batch leaves half of the CUs without a 256 x 256
    // tile (ImageNet-256 latents: 32 x 4 tiles): a function of the model (max_batch), never of a call's batch
    m->splitk = precision == DD_PREC_BF16 && !m->fused_mlp && !m->rowlin_fc2 && D % 256 == 0 && !(flags & DD_DEV_NO_SPLITK) &&
                (long long)(m->cfg.max_batch * L / 256) * (D / 256) * 2 <= device_num_cus() &&
                (hid / 64) % 2 == 0;
    for (int b = 1; m->splitk && b <= m->cfg.max_batch; ++b)     // every batch this model can be called with must fit the kernel's row partition
        m->splitk = gemm_splitk_supported(b * L, D, D, D, 2);
}

const std::vector<float>& param(const dd_model* m, const std::string& name) { return m->params.at(name).data; }

// block bi into m->blocks[bi].  next_skip: prefix of the block whose skip_linear runs in THIS block's fused launch ("" = none);
// next_qkv: prefix of the block whose attn.qkv runs in THIS block's fused launch ("" = none: the last block)
void pack_block(dd_model* m, Arena& a, int bi, const std::string& next_skip, const std::string& next_qkv) {
    const int D = m->D, hid = m->hidden;
    const std::string p = block_prefix(m, bi);
    auto P = [&](const std::string& n) -> const std::vector<float>& { return param(m, n); };
    BlockW& w = m->blocks[bi];
    a.f32(w.ln1_g, P(p + "norm1.weight")); a.f32(w.ln1_b, P(p + "norm1.bias"));
    a.f32(w.ln2_g, P(p + "norm2.weight")); a.f32(w.ln2_b, P(p + "norm2.bias"));
    a.f32(w.proj_b, P(p + "attn.proj.bias"));
    a.f32(w.fc1_b, P(p + "mlp.fc1.bias")); a.f32(w.fc2_b, P(p + "mlp.fc2.bias"));
    a.mat(w.qkv_w, P(p + "attn.qkv.weight")); a.mat(w.proj_w, P(p + "attn.proj.weight"));
    if (m->cfg.qkv_bias) a.f32(w.qkv_b, P(p + "attn.qkv.bias"));
    a.mat(w.fc1_w, P(p + "mlp.fc1.weight")); a.mat(w.fc2_w, P(p + "mlp.fc2.weight"));
    const bool skip = bi > m->half_depth;
    if (skip) { a.f32(w.skip_b, P(p + "skip_linear.bias")); a.mat(w.skip_w, P(p + "skip_linear.weight")); }
    if (m->fused_mlp) {
        const bool with_skip = m->fused_skip && !next_skip.empty();
        // (an out-block's qkv needs its skip_linear in here too; with fused_qa the attention launch computes qkv and no section is packed)
        const bool with_qkv = m->fused_qkv && !m->fused_qa && !next_qkv.empty() && (next_skip.empty() || with_skip);
        const TailImage t = pack_tail_image(D, hid, m->fused_proj ? P(p + "attn.proj.weight").data() : nullptr, P(p + "mlp.fc1.weight").data(),
                                            P(p + "mlp.fc1.bias").data(), P(p + "mlp.fc2.weight").data(), true,
                                            with_skip ? P(next_skip + "skip_linear.weight").data() : nullptr,      // the next block's skip_linear
                                            with_qkv ? P(next_qkv + "attn.qkv.weight").data() : nullptr);          // the next block's attn.qkv
        std::memcpy(a.raw(w.mlp_img, t.img.size() * 2), t.img.data(), t.img.size() * 2);
        a.f32(w.mlp_b1p, t.b1p);
    }
    if (m->fused_qa)
        qkv_attention_pack(D, m->H, P(p + "attn.qkv.weight").data(), host_f2bf, (unsigned short*)a.raw(w.qa_img, (size_t)3 * D * D * 2));
    if (m->rowlin_fc2) {
        rowlin_pack(hid, P(p + "mlp.fc2.weight").data(), host_f2bf, (unsigned short*)a.raw(w.rl_img, (size_t)D * hid * 2));
        rowlin_pack(D, P(p + "attn.proj.weight").data(), host_f2bf, (unsigned short*)a.raw(w.rlp_img, (size_t)D * D * 2));
        if (skip) rowlin_pack(2 * D, P(p + "skip_linear.weight").data(), host_f2bf, (unsigned short*)a.raw(w.rls_img, (size_t)D * 2 * D * 2));
    }
}

// patch, position and label embeddings and the time_embed MLP
void pack_embed(dd_model* m, Arena& a) {
    const int D = m->D, pd = m->pd;
    auto P = [&](const std::string& n) -> const std::vector<float>& { return param(m, n); };
    // patch-embed weight [D, pd] -> transposed [pd, D] (coalesced over D in the embed kernel)
    a.f32(m->emb_wt, transposed(P("patch_embed.proj.weight").data(), D, pd)); a.f32(m->emb_b, P("patch_embed.proj.bias")); a.f32(m->pos, P("pos_embed"));
    if (m->cfg.num_classes > 0) a.f32(m->label, P("label_emb.weight"));
    if (m->cfg.mlp_time_embed) {   // transposed: the kernel's threads run over the OUTPUT index
        a.f32(m->tm_w1t, transposed(P("time_embed.0.weight").data(), 4 * D, D)); a.f32(m->tm_b1, P("time_embed.0.bias"));
        a.f32(m->tm_w2t, transposed(P("time_embed.2.weight").data(), D, 4 * D)); a.f32(m->tm_b2, P("time_embed.2.bias"));
    }
}

// an output head (state_dict prefix p; "" = the final head) into h: LayerNorm, decoder_pred, final_layer.  fused: the head_dec_kernel
// operands too, the norm folded into decoder_pred (dec = (W . diag(gamma)) xn + (b + W . beta)); split: and Wg as hi + lo bf16 halves in
// the SPLIT kernel's fragment order
void pack_head(const dd_model* m, Arena& a, const std::string& p, HeadW& h, bool fused, bool split) {
    const int D = m->D, pd = m->pd;
    auto P = [&](const std::string& n) -> const std::vector<float>& { return param(m, n); };
    const std::vector<float>&ng = P(p + "norm.weight"), &nb = P(p + "norm.bias"), &wd = P(p + "decoder_pred.weight"), &bd = P(p + "decoder_pred.bias");
    a.f32(h.ng, ng); a.f32(h.nb, nb); a.f32(h.wdec, wd); a.f32(h.bdec, bd);
    a.f32(h.wconv, P(p + "final_layer.weight")); a.f32(h.bconv, P(p + "final_layer.bias"));
    if (!fused) return;
    const HeadImage hi = pack_head_image(D, pd, wd.data(), bd.data(), ng.data(), nb.data(), split);
    a.f32(h.wg, hi.wg); a.f32(h.dc, hi.dc);
    if (!split) return;
    std::memcpy(a.raw(h.wsplit, hi.wsplit.size() * 2), hi.wsplit.data(), hi.wsplit.size() * 2);
    a.f32(h.dcs, hi.dcs);
}

// the early-exit probes: one AttentionProbe per layer, or the [n_probe, D] / [n_probe] table of the MLP probes
void pack_probes(dd_model* m, Arena& a) {
    const int D = m->D;
    auto P = [&](const std::string& n) -> const std::vector<float>& { return param(m, n); };
    int nt, nl;
    probe_grid(m, nt, nl);
    if (m->ee_type == DD_EE_ATTENTION_PROBE) {
        // AttentionProbe (early_exit.py:40-80), one learned query, one head: the operands folded by fold_attn_probe (launch_args.h)
        m->attn_probes.resize(nl);
        for (int layer = 0; layer < nl; ++layer) {
            const std::string pre = "matrix." + probe_key(m, layer, 0) + ".";
            const std::vector<float>&q = P(pre + "q"), &wkv = P(pre + "weight_kv.weight"), &bkv = P(pre + "weight_kv.bias"),
                                    &w0 = P(pre + "classification.0.weight");
            const AttnProbeFold f = fold_attn_probe(D, q.data(), wkv.data(), w0.data());
            AttnProbeW& w = m->attn_probes[layer];
            a.f32(w.u, f.u); a.f32(w.wvt, f.wvt); a.f32(w.bv, bkv.data() + D, D);
            a.f32(w.w0t, f.w0t); a.f32(w.b0, P(pre + "classification.0.bias"));
            a.f32(w.w2, P(pre + "classification.2.weight")); a.f32(w.b2, P(pre + "classification.2.bias"));
        }
        return;
    }
    m->n_probe = nt * nl;
    std::vector<float> pw((size_t)m->n_probe * D), pb(m->n_probe);
    for (int t = 0; t < nt; ++t)
        for (int layer = 0; layer < nl; ++layer) {
            const std::string pre = "matrix." + probe_key(m, layer, t) + ".classifier.0.";
            const int row = t * nl + layer;
            std::memcpy(&pw[(size_t)row * D], P(pre + "weight").data(), (size_t)D * 4);
            pb[row] = P(pre + "bias")[0];
        }
    a.f32(m->probe_w, pw); a.f32(m->probe_b, pb);
}

}  // namespace

namespace dd {
// (zeroed ON THE LAUNCH STREAM: the second chain's stream is non-blocking, so a null-stream memset is not ordered before its first kernels --
// the chain's first step ran while the memset was still sweeping the arena: the first images of the second half came out wrong on the very
// first chained call of a model, intermittently)
int ensure_chain_ws(dd_ctx* c, dd_model* m, hipStream_t s) {
    if (m->wsarena[1]) return DD_OK;
    Arena a;
    ws_layout(m, (m->cfg.max_batch + 1) / 2, m->ws[1], a);     // a chain never runs more than half of max_batch
    m->ws_bytes[1] = a.bytes();
    DD_HIP(c, hipMalloc((void**)&m->wsarena[1], m->ws_bytes[1]));
    DD_HIP(c, hipMemsetAsync(m->wsarena[1], 0, m->ws_bytes[1], s));
    a.bind(m->wsarena[1]);
    return DD_OK;
}
// (chain 1's is laid out for half of max_batch, as its workspace; zeroed on the launch stream for the reason above: the GEMMs read whole
// tiles of rows, the rows past the batch's included)
int ensure_block_cache(dd_ctx* c, dd_model* m, int chain, hipStream_t s) {
    BlockCache& bc = m->cache[chain];
    if (bc.last) return DD_OK;
    const size_t bytes = (size_t)round_up((chain ? (m->cfg.max_batch + 1) / 2 : m->cfg.max_batch) * m->L, 256) * m->D * m->esize;
    for (void** p : {&bc.last, &bc.prev, &bc.yhat}) {
        DD_HIP(c, hipMalloc(p, bytes));
        DD_HIP(c, hipMemsetAsync(*p, 0, bytes, s));
    }
    return DD_OK;
}
}  // namespace dd

// ==========================================================================================
extern "C" {

int dd_schedule_table(int which, float* out) {
    if (!out) return DD_ERR_INVALID;
    const Schedule& s = schedule();
    const float* src = nullptr;
    switch (which) {
        case 0: src = s.betas; break;
        case 1: src = s.alphas; break;
        case 2: src = s.abar; break;
        case 3: src = s.abar_prev; break;
        case 4: src = s.bt_sampler; break;
        case 5: src = s.bt_sched; break;
        case 6: src = s.c1; break;
        case 7: src = s.c2; break;
        case 8: src = s.sigma; break;
        default: return DD_ERR_INVALID;
    }
    std::memcpy(out, src, 1000 * sizeof(float));
    return DD_OK;
}

int dd_schedule_build(float beta_init, float beta_final, int steps, float* betas, float* alphas, float* alphas_bar,
                      float* alphas_bar_prev, float* betas_tilde) {
    if (steps < 1 || steps > (1 << 20)) return DD_ERR_INVALID;
    std::vector<float> b(steps), a(steps), ab(steps), abp(steps);
    base_tables(beta_init, beta_final, steps, b.data(), a.data(), ab.data(), abp.data());
    const size_t bytes = (size_t)steps * sizeof(float);
    if (betas) std::memcpy(betas, b.data(), bytes);
    if (alphas) std::memcpy(alphas, a.data(), bytes);
    if (alphas_bar) std::memcpy(alphas_bar, ab.data(), bytes);
    if (alphas_bar_prev) std::memcpy(alphas_bar_prev, abp.data(), bytes);
    if (betas_tilde)
        for (int i = 0; i < steps; ++i) betas_tilde[i] = bt_scheduler_order(b[i], abp[i], ab[i]);
    return DD_OK;
}

int dd_model_create(dd_ctx* c, const dd_config* cfg, dd_model** out) {
    if (!c || !cfg || !out) return DD_ERR_INVALID;
    *out = nullptr;
    const dd_config& g = *cfg;
    if (g.img_size <= 0 || g.patch_size <= 0 || g.img_size % g.patch_size) return ctx_fail(c, DD_ERR_INVALID, "img_size must be a positive multiple of patch_size");
    if (g.num_heads <= 0 || g.embed_dim != g.num_heads * 64) return ctx_fail(c, DD_ERR_UNSUPPORTED, "kernels require head_dim == 64 (all shipped configs)");
    if (g.depth < 1 || g.depth % 2 != 1) return ctx_fail(c, DD_ERR_INVALID, "depth must be odd");
    if (g.in_chans < 1 || g.in_chans > 4) return ctx_fail(c, DD_ERR_UNSUPPORTED, "in_chans must be 1..4");
    if (g.embed_dim > 1024) return ctx_fail(c, DD_ERR_UNSUPPORTED, "embed_dim must be <= 1024");
    if (g.max_batch < 1) return ctx_fail(c, DD_ERR_INVALID, "max_batch must be >= 1");
    dd_model* m = new (std::nothrow) dd_model();
    if (!m) return ctx_fail(c, DD_ERR_NOMEM, "out of host memory");
    m->ctx = c; m->cfg = g;
    m->D = g.embed_dim; m->H = g.num_heads;
    m->N = (g.img_size / g.patch_size) * (g.img_size / g.patch_size);
    m->extras = g.num_classes > 0 ? 2 : 1;
    m->L = m->N + m->extras;
    m->pd = g.patch_size * g.patch_size * g.in_chans;
    m->pdp = round_up(m->pd, 8);
    m->hidden = g.embed_dim * (g.mlp_ratio > 0 ? g.mlp_ratio : 4);
    m->hid_ld = m->hidden;   // row stride of the MLP hidden activation (a +64 pad against power-of-two strides measured no gain)
    m->half_depth = g.depth / 2;
    m->Mp_max = round_up(g.max_batch * m->L, 256);
    // (L <= 288: attention_kernel, K and V of a head in one LDS image; beyond: attention_long_kernel streams them, launch_attention_long's bound)
    if (m->N > kMaxLongL - 2) { delete m; return ctx_fail(c, DD_ERR_UNSUPPORTED, "(img_size / patch_size)^2 must be <= 4096 patches"); }
    // the head-major row map of the qkv Linear (hm_offset) divides a row index by L with a 32-bit multiply: exact while rows x L < 2^32.  Below 289
    // tokens that is a batch of 51 781 and stays the launch's own check; beyond, it is within reach (255 images of 4098 tokens) and is refused here
    if (m->L > 288 && (long long)g.max_batch * m->L * m->L >= (1ll << 32)) {
        delete m;
        return ctx_fail(c, DD_ERR_UNSUPPORTED, "above 288 tokens max_batch x tokens^2 must be < 2^32 (" + std::to_string((1ll << 32) / ((long long)m->L * m->L)) + " images at this size)");
    }
    if (m->pd > 64) { delete m; return ctx_fail(c, DD_ERR_UNSUPPORTED, "patch_size^2 * in_chans must be <= 64"); }
    m->params = catalogue(m);
    static std::atomic<unsigned long long> serials{0};
    m->serial = ++serials;
    *out = m;
    return DD_OK;
}

int dd_model_set_param(dd_model* m, const char* name, const float* host, const int64_t* shape, int ndim) {
    if (!m || !name || !host || !shape || ndim < 1) return DD_ERR_INVALID;
    dd_ctx* c = m->ctx;
    if (m->finalized) return ctx_fail(c, DD_ERR_STATE, "model already finalized");
    auto it = m->params.find(name);
    if (it == m->params.end()) return ctx_fail(c, DD_ERR_NOT_FOUND, std::string("unexpected key in state_dict: ") + name);
    HostParam& p = it->second;
    const std::vector<int64_t>& want = p.shape;
    std::vector<int64_t> got(shape, shape + ndim);
    if (got != want) {
        std::string msg = std::string("size mismatch for ") + name + ": expected [";
        for (size_t i = 0; i < want.size(); ++i) msg += (i ? "," : "") + std::to_string(want[i]);
        msg += "], got [";
        for (size_t i = 0; i < got.size(); ++i) msg += (i ? "," : "") + std::to_string(got[i]);
        return ctx_fail(c, DD_ERR_INVALID, msg + "]");
    }
    size_t n = 1;
    for (auto d : want) n *= (size_t)d;
    p.data.assign(host, host + n);
    p.set = true;
    return DD_OK;
}

int64_t dd_model_num_params(const dd_model* m) {
    if (!m) return 0;
    int64_t n = 0;
    for (auto& kv : m->params) n += (int64_t)kv.second.data.size();
    return n;
}

int dd_model_finalize(dd_model* m, int precision) {
    if (!m) return DD_ERR_INVALID;
    dd_ctx* c = m->ctx;
    if (m->finalized) return ctx_fail(c, DD_ERR_STATE, "model already finalized");
    if (precision != DD_PREC_BF16 && precision != DD_PREC_FP32) return ctx_fail(c, DD_ERR_INVALID, "unknown precision");
    for (const auto& kv : m->params)
        if (!kv.second.set) return ctx_fail(c, DD_ERR_NOT_FOUND, "missing key in state_dict: " + kv.first);
    DD_HIP(c, hipSetDevice(c->device));
    m->prec = precision;
    m->esize = precision == DD_PREC_BF16 ? 2 : 4;
    choose_paths(m, precision, c->dev_flags);
    const int depth = m->cfg.depth, L = m->L;

    // ---- pack weights into one arena: fp32 vectors/tables + T-typed GEMM matrices
    Arena w(m->esize);
    m->blocks.resize(depth);   // (sized before any slot is taken: the arena binds their fields in place)
    for (int bi = 0; bi < depth; ++bi) {
        const std::string next = bi + 1 < depth ? block_prefix(m, bi + 1) : "";
        pack_block(m, w, bi, bi + 1 > m->half_depth ? next : "", next);   // (only out-blocks have a skip_linear)
    }
    pack_embed(m, w);
    const bool fused_head = head_dec_supported(m->D, m->pd) && !(c->dev_flags & DD_DEV_NO_FUSED_HEAD);
    pack_head(m, w, "", m->head, fused_head, false);
    if (m->ee_type >= 0) {   // the early-exit heads: identical consecutive records (ee_conv_stride_ok), split-bf16 in the bf16 engine
        const bool split_heads = fused_head && m->esize == 2 && head_dec_probe_supported(m->D) && !(c->dev_flags & DD_DEV_NO_SPLIT_HEADS);
        m->heads.resize(depth);
        for (int layer = 0; layer < depth; ++layer) pack_head(m, w, head_prefix(m, layer), m->heads[layer], fused_head, split_heads);
        pack_probes(m, w);
    }
    DD_HIP(c, hipMalloc((void**)&m->warena, w.bytes()));
    DD_HIP(c, hipMemcpy(m->warena, w.image(), w.bytes(), hipMemcpyHostToDevice));
    w.bind(m->warena);

    if (m->heads.size() >= 2) {
        m->ee_wconv_stride = m->heads[1].wconv - m->heads[0].wconv; m->ee_bconv_stride = m->heads[1].bconv - m->heads[0].bconv;
        m->ee_conv_stride_ok = true;
        for (size_t i = 0; i < m->heads.size(); ++i)
            if (m->heads[i].wconv != m->heads[0].wconv + (long long)i * m->ee_wconv_stride || m->heads[i].bconv != m->heads[0].bconv + (long long)i * m->ee_bconv_stride) m->ee_conv_stride_ok = false;
    }
    // the batched early-exit heads need nb B L (pd + 1) floats of the MLP hidden buffer: decided here for both chain workspaces (the need
    // grows linearly in B, so it then fits every call) and never from a call's B, so that an image's probe value does not depend on its batch
    auto ee_fits = [&](int b) {
        return m->blocks.size() * b * L * (m->pd + 1) * sizeof(float) <= (size_t)round_up(b * L, 256) * m->hid_ld * m->esize;
    };
    m->ee_batched = m->ee_type >= 0 && precision == DD_PREC_BF16 && m->fused_mlp && m->ee_conv_stride_ok && m->heads[0].wg &&
                    ee_fits(m->cfg.max_batch) && ee_fits((m->cfg.max_batch + 1) / 2);

    // ---- activation workspace (HBM-resident for the life of the model)
    Arena a;
    ws_layout(m, m->cfg.max_batch, m->ws[0], a);
    m->ws_bytes[0] = a.bytes();
    DD_HIP(c, hipMalloc((void**)&m->wsarena[0], m->ws_bytes[0]));
    DD_HIP(c, hipMemset(m->wsarena[0], 0, m->ws_bytes[0]));
    DD_HIP(c, hipStreamSynchronize(nullptr));    // (callers run the model on non-blocking streams, which a null-stream memset does not order itself before)
    a.bind(m->wsarena[0]);

    // host copies are no longer needed
    for (auto& kv : m->params) { std::vector<float>().swap(kv.second.data); }
    m->finalized = true;
    return DD_OK;
}

void dd_model_destroy(dd_model* m) {
    if (!m) return;
    (void)hipSetDevice(m->ctx->device);
    for (auto& kind : m->graph)
        for (hipGraphExec_t g : kind) if (g) (void)hipGraphExecDestroy(g);
    for (hipEvent_t e : m->fc1_events) (void)hipEventDestroy(e);
    if (m->ee_ws) (void)hipFree(m->ee_ws);
    if (m->real_tabs) (void)hipFree(m->real_tabs);
    if (m->real_counts_host) (void)hipHostFree(m->real_counts_host);
    for (hipEvent_t e : m->real_ev) if (e) (void)hipEventDestroy(e);
    for (BlockCache& bc : m->cache)
        for (void* p : {bc.last, bc.prev, bc.yhat}) if (p) (void)hipFree(p);
    if (m->warena) (void)hipFree(m->warena);
    for (char* a : m->wsarena) if (a) (void)hipFree(a);
    delete m;
}

int dd_model_enable_early_exit(dd_model* m, int classifier_type) {
    if (!m) return DD_ERR_INVALID;
    dd_ctx* c = m->ctx;
    const bool any_set = std::any_of(m->params.begin(), m->params.end(), [](const auto& kv) { return kv.second.set; });
    if (m->finalized || any_set) return ctx_fail(c, DD_ERR_STATE, "enable early exit before any parameter is set");
    if (classifier_type < DD_EE_MLP_PER_LAYER || classifier_type > DD_EE_ATTENTION_PROBE)
        return ctx_fail(c, DD_ERR_UNSUPPORTED, "unknown classifier type");
    if (m->L > 288) return ctx_fail(c, DD_ERR_UNSUPPORTED, "early-exit models: sequence length must be <= 288 tokens");
    m->ee_type = classifier_type;
    m->params = catalogue(m);   // the heads and probes of this classifier type
    return DD_OK;
}

int dd_dev_poison_workspaces(dd_ctx* c, dd_model* m, void* stream) {
    if (!c || !m || m->ctx != c || !m->finalized) return DD_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = ensure_chain_ws(c, m, s)) return rc;
    for (int k = 0; k < 2; ++k) DD_HIP(c, hipMemsetAsync(m->wsarena[k], 0xFF, m->ws_bytes[k], s));
    // the context's model-output scratch of the thresholded loop, sized for this model's largest batch (it only grows)
    if (int rc = c->m_stage.grow(c, (size_t)m->cfg.max_batch * m->cfg.in_chans * m->cfg.img_size * m->cfg.img_size)) return rc;
    DD_HIP(c, hipMemsetAsync(c->m_stage.p, 0xFF, c->m_stage.n * sizeof(float), s));
    return DD_OK;
}

}  // extern "C"
