// extern "C" surface of libduodiff.so (include/duodiff.h): context, model packing, the U-ViT
// forward as a sequence of HIP kernels, the fused sampling step and the hipGraph-replayed loop.
//
// Host-side restatement of: UViT.__init__ / forward wiring (reference models/uvit.py:228-383),
// get_samples DDPM branch and backbone switch (sampler.py:128-139), schedule constants
// (sampler.py:40-44, ddpm_core.py:64-70).
#include "../../include/duodiff.h"
#include "../../include/duodiff_dev.h"
#include "dd_internal.h"
#include "dev_scope.h"
#include "host_arena.h"
#include "launch_args.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <new>
#include <string>
#include <vector>

using namespace dd;

namespace dd {
hipError_t init_gemm_kernels();
hipError_t init_attention_kernels();
hipError_t init_rowops_kernels();
int device_num_cus();
}  // namespace dd

#define DD_HIP(c, expr)                                          \
    do {                                                         \
        hipError_t _e = (expr);                                  \
        if (_e != hipSuccess) return fail_hip((c), _e, #expr);   \
    } while (0)

namespace {
// A device buffer of the context that only grows: a captured step is keyed on its address, so graphs are re-captured once after it grew
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;        // elements
    int grow(dd_ctx* c, size_t need) {       // the old block is freed first; a failed allocation leaves the buffer empty
        if (n >= need) return DD_OK;
        release();
        DD_HIP(c, hipMalloc((void**)&p, need * sizeof(T)));
        n = need;
        return DD_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr; n = 0;
    }
};
// A table of per-step rows on the device with the host copy it is uploaded from (upload_rows)
template <typename Row>
struct RowTable {
    DevBuf<Row> dev;
    std::vector<Row> host;
    hipEvent_t uploaded = nullptr;      // behind the last upload: the host copy is not rewritten before it has been read
    void release() {
        dev.release();
        if (uploaded) (void)hipEventDestroy(uploaded);
        uploaded = nullptr;
    }
};
}  // namespace

// ------------------------------------------------------------------------------------------
struct dd_ctx {
    int device = 0;
    std::string err;
    StepState* st[2] = {nullptr, nullptr};   // device: the step state (timestep / counter) of each half-batch chain (Chain)
    hipStream_t side = nullptr;  // the second chain's stream (context-owned, non-blocking)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev_ee_fork = nullptr, ev_ee_join = nullptr;   // early-exit heads / probes of a layer on the side stream, beside the block's attention launch
    StepCoef* coef = nullptr;    // device [1000]
    StepCoef coef_host[1000];
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    float timing[3] = {0, 0, 0};
    int num_cus = 256;           // CU count the persistent GEMM grids are sized for (dd_set_num_cus), a multiple of 8
    // dd_sample's graphs run on context-owned staging copies of x / y, so a captured step does not depend on the caller's
    // tensor addresses (reference get_samples allocates a fresh x per call: the graphs would be re-captured every time)
    DevBuf<float> x_stage;
    DevBuf<int64_t> y_stage;
    long long graph_captures = 0;
    int last_chains = 1;         // chains the last dd_sample call ran (dd_dev_last_sample_chains)
    RowTable<AffineRow> atab;    // dd_sample_affine: the step table
    RowTable<HistRow> htab;      // dd_sample_multistep: the history half of the rows beside atab,
    DevBuf<float> h_stage;       //   and the history register the loop runs on ([B, C, S, S], staged like x)
    RowTable<KnownRow> ktab;     // the *_region loops: the known-region half of the rows,
    DevBuf<float> k_stage;       //   and the known image and mask the loop reads (x0 [B, C, S, S] | mask [B, 1, S, S], staged like x)
    DevBuf<float> m_stage;       // dd_sample_multistep_threshold: the step's (guided) model output [B, C, S, S], chain k's images at its first image:
                                 //   written by the output head and read by threshold_step_kernel within one step, never across steps
    int prof_kind = 0;           // dd_profile_select: which launches dd_profile_steps brackets (DD_PROF_*)
    unsigned dev_flags = 0;      // dd_dev_set_flags (include/duodiff_dev.h): kernel-variant switches of the development harness
};

namespace {

struct HostParam {
    std::vector<float> data;
    std::vector<int64_t> shape;
    bool set = false;
};

struct BlockW {
    const float *ln1_g, *ln1_b, *ln2_g, *ln2_b, *proj_b, *fc1_b, *fc2_b, *skip_b, *qkv_b;
    const void *qkv_w, *proj_w, *fc1_w, *fc2_w, *skip_w;
    const char* mlp_img;     // fused-MLP weight image (mlp_fused.hip) or null
    const float* mlp_b1p;    // fc1 bias in accumulator-register order
    const bf16_t* qa_img;    // attn.qkv weight per head in fragment order (qkv_attention_pack) or null
    const char* rl_img = nullptr;   // mlp.fc2 weight as the row-resident launch streams it (rowlin_pack) or null
    const char* rlp_img = nullptr;  // attn.proj weight, ditto
    const char* rls_img = nullptr;  // skip_linear weight [D, 2 D], ditto (out-blocks)
};

struct HeadW { const float *ng, *nb, *wdec, *bdec, *wconv, *bconv; const float *wg = nullptr, *dc = nullptr; const float *wsplit = nullptr, *dcs = nullptr; };   // wg / dc: head_dec_kernel operands (norm folded into decoder_pred; dc = c [pd], row sums of wg [pd]) or null; wsplit / dcs: the same for the split-bf16 product (bf16 engine, embed_dim 256 / 512) or null

struct GraphKey {
    const void* x; const void* y; int B, noise, variance, num_cus;   // num_cus: the captured persistent grids are sized from it
    const void* atab;                                                // dd_sample_affine's table (null: the DDPM update)
    const void *aux0 = nullptr, *aux1 = nullptr;                     // dd_sample_early_exit: the two log tables
    float thr = 0.f;                                                 //                        and the threshold
    int b0 = 0;                                                      // first image of a half-batch chain within the whole batch
    int gnull = -1;                                                  // classifier-free guidance: the null label (-1: unguided)
    unsigned gscale = 0;                                             //   and the bits of the scale (+0 and -0 round differently)
    const void* aguide = nullptr;                                    // autoguidance: the guide model of a two-model step (null: CFG / unguided; gscale: the scale's bits)
    unsigned long long aserial = 0;                                  //   and its serial: an address can come back with another model behind it
    const void *kx0 = nullptr, *kmask = nullptr, *ktab = nullptr;    // known region: the chain's staged x0 / mask and the rows (null: none)
    int tmode = -1;                                                  // x0 thresholding: the mode (-1: none), the bits of quantile, range and s_max,
    unsigned tq = 0, tr = 0, ts = 0;                                 //   and the model-output scratch the step goes through
    const void* tscratch = nullptr;
    int pag = 0;                                                     // perturbed-attention guidance: set (gscale: the scale's bits), and the
    unsigned pfirst = 0, plate = 0;                                  //   masks of the loop's two models
    bool operator==(const GraphKey& o) const {
        return x == o.x && y == o.y && B == o.B && noise == o.noise && variance == o.variance && num_cus == o.num_cus &&
               atab == o.atab && aux0 == o.aux0 && aux1 == o.aux1 && thr == o.thr && b0 == o.b0 && gnull == o.gnull && gscale == o.gscale &&
               aguide == o.aguide && aserial == o.aserial && kx0 == o.kx0 && kmask == o.kmask && ktab == o.ktab && tmode == o.tmode &&
               tq == o.tq && tr == o.tr && ts == o.ts && tscratch == o.tscratch && pag == o.pag && pfirst == o.pfirst && plate == o.plate;
    }
    void perturb(const dd_pag* p) {
        if (p) { pag = 1; gscale = __builtin_bit_cast(unsigned, p->scale); pfirst = p->layers_first; plate = p->layers_late; }
    }
    void guide(const dd_guidance* g) {
        if (g) { gnull = g->null_label; gscale = __builtin_bit_cast(unsigned, g->scale); }
    }
};

// the captured step of each sampling loop: dd_model::graph[kind][chain]
enum GraphKind { GRAPH_DDPM, GRAPH_AFFINE, GRAPH_EARLY_EXIT, GRAPH_MULTISTEP, GRAPH_KINDS };

}  // namespace

// The activation workspace of one chain: dd_sample runs a large batch as TWO independent half-batch chains on two streams (one
// chain's HBM-bound kernel phases then run under the other's MFMA phases); the second chain has its own copy of every buffer.
struct WsPtrs {
    float* x = nullptr; void *h = nullptr, *ao = nullptr, *qkv = nullptr, *hid = nullptr, *xb = nullptr;
    std::vector<void*> skips;
    float* dec = nullptr;
    float* mlp_partial = nullptr;         // partial slabs of hidden-split leftover tiles (mlp_fused_plan)
    bf16_t* qkv_dump = nullptr;           // scratch for the qkv stores of rows past the end of a ragged tile
    bf16_t* hfrag = nullptr;              // fused_qa: norm1 of the patch rows in MFMA fragment order (MlpFusedArgs::ln_out_frag)
    // the patch rows' hand-offs in MFMA fragment order (dd_model::frag_ao / frag_skip / frag_x): each buffer holds batch * N * D elements
    bf16_t* aofrag = nullptr;             // attention output -> the tail's projection (QkvAttnArgs::out_frag -> MlpFusedArgs::ao_frag)
    std::vector<bf16_t*> skipfrags;       // in-block bi's bf16 copy -> the SKIP phases of its out-block's tail (out_frag -> skip_frag)
    float* xfrag = nullptr;               // the fp32 residual rows from one tail to the next (x_out_frag -> x_in_frag)
    float* ytap = nullptr;                // early-exit models with fused_skip: the block output y of the launches that run the next skip_linear (MlpFusedArgs::y_tap)
};

struct dd_model {
    dd_ctx* ctx = nullptr;
    unsigned long long serial = 0;   // unique per dd_model_create of the process (graph keys that name another model: autoguidance)
    dd_config cfg{};
    int D = 0, L = 0, N = 0, extras = 0, pd = 0, pdp = 0, H = 0, hidden = 0, hid_ld = 0, half_depth = 0, Mp_max = 0;
    std::map<std::string, HostParam> params;   // every state_dict name of the model (catalogue), its data once set (dropped by finalize)
    bool finalized = false;
    int prec = DD_PREC_BF16;
    size_t esize = 2;
    char* warena = nullptr;    // weights
    std::vector<BlockW> blocks;  // in.., mid, out..
    const float *emb_wt = nullptr, *emb_b = nullptr, *pos = nullptr, *label = nullptr;
    const float *tm_w1t = nullptr, *tm_b1 = nullptr, *tm_w2t = nullptr, *tm_b2 = nullptr;   // time_embed MLP (mlp_time_embed)
    HeadW head{};                         // the final head (uvit.py:377-380; no split-bf16 image)
    // early-exit baseline (models/early_exit.py:193-268): per-layer output heads + MLP probes; ee_type < 0: plain U-ViT
    int ee_type = -1, n_probe = 0;
    std::vector<HeadW> heads;             // head i is applied to the input of block i
    const float *probe_w = nullptr, *probe_b = nullptr;   // [n_probe, D], [n_probe]
    std::vector<AttnProbeW> attn_probes;                  // DD_EE_ATTENTION_PROBE: one per layer
    bool ee_conv_stride_ok = false;                       // the heads' conv weights / biases sit at a constant stride in the weight arena (one batched conv launch)
    long long ee_wconv_stride = 0, ee_bconv_stride = 0;
    bool ee_batched = false;                              // early-exit heads / probes batched behind the last block (Backbone::ee_dec_all)
    bool fused_mlp = false;               // bf16 mode, D in {64,128,256,512}: fc1+GELU+fc2+residual in one launch
    bool fused_proj = false;              // ... and attn.proj + residual in front of it (D % 128 == 0): patch rows only
    bool fused_skip = false;              // ... and the NEXT block's skip_linear + norm1 behind it (mid / out blocks; early-exit models tap y on the way,
                                          //     whose heads read every block's output)
    bool fused_qkv = false;               // ... and the NEXT block's attn.qkv Linear last of all (no qkv bias; not for early-exit models)
    bool splitk = false;                  // GEMM-path models whose N = embed_dim Linears have too few 256 x 256 tiles at max_batch: split-K + reduce_ln launches
    bool rowlin_skip = false;             // ... and the out-blocks' skip_linear + norm1
    bool rowlin_proj = false;             // ... and attn.proj + residual + norm2 likewise
    bool rowlin_fc2 = false;              // embed_dim 768 on the GEMM path: mlp.fc2 + residual + the next block's norm1 in one row-resident launch (rowlin.hip)
    // fused_qa + fused_proj at embed_dim 512: the patch rows travel between the attention launch and the block tails in fragment order, 1 KB per wave
    // instruction on both sides; the extra-token rows stay row-major in ao / skips / x
    bool frag_ao = false;                 // attention output -> projection
    bool frag_skip = false;               // in-block output -> the out-block's skip_linear (fused_skip)
    bool frag_x = false;                  // residual rows between consecutive tails (not for early-exit models, whose heads read x every block)
    bool fused_qa = false;                // attn.qkv computed inside the attention launch (attention.hip qkv_attention_kernel): takes precedence over
                                          // fused_qkv wherever the previous block's fused launch leaves norm1 in h
    // each chain's activation workspace: [0] laid out for max_batch (dd_model_finalize), [1] for half of it (ensure_chain_ws, on the first chained call)
    size_t ws_bytes[2] = {0, 0};
    char* wsarena[2] = {nullptr, nullptr};
    WsPtrs ws[2];
    hipGraphExec_t graph[GRAPH_KINDS][2] = {};                // each loop's captured step, per chain
    GraphKey gkey[GRAPH_KINDS][2]{};
    float* ee_ws = nullptr;                                  // dd_sample_early_exit scratch: eps | cls | outs (two chains: one such block per chain, half the batch each),
                                                             // then the chains' per-step sums of the predicted errors [2][1000][depth]
    // in-context timing (dd_profile_steps): event pairs recorded around each launch of kind ctx->prof_kind when enabled
    bool time_fc1 = false;
    std::vector<hipEvent_t> fc1_events;   // pairs, grown on demand
    size_t fc1_used = 0;
};

namespace dd {
// declared in dev_scope.h for vae.hip and dev_harness.hip (dd_ctx is defined in this translation unit)
int ctx_fail(dd_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}
int ctx_device(dd_ctx* c) { return c->device; }
int ctx_num_cus(dd_ctx* c) { return c->num_cus; }
unsigned ctx_dev_flags(dd_ctx* c) { return c->dev_flags; }
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

struct Schedule {
    float betas[1000], alphas[1000], abar[1000], abar_prev[1000], bt_sampler[1000], bt_sched[1000];
    float c1[1000], c2[1000], sigma[1000], sigma_beta[1000];
    Schedule() {
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
};
const Schedule& schedule() {
    static const Schedule s;
    return s;
}

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
        // AttentionProbe (early_exit.py:40-80), one learned query, one head.  q . (Wk x + bk) = (Wk^T q) . x + const, and the
        // constant cancels in the softmax; sum_l p_l (Wv x_l + bv) = Wv (sum_l p_l x_l) + bv.  So the probe needs u = Wk^T q /
        // sqrt(D) (folded here, in double), and Wv / classification.0 transposed for coalesced mat-vecs -- never the [L, 2D] kv.
        m->attn_probes.resize(nl);
        for (int layer = 0; layer < nl; ++layer) {
            const std::string pre = "matrix." + probe_key(m, layer, 0) + ".";
            const std::vector<float>&q = P(pre + "q"), &wkv = P(pre + "weight_kv.weight"), &bkv = P(pre + "weight_kv.bias"),
                                    &w0 = P(pre + "classification.0.weight");
            std::vector<float> u(D), wvt((size_t)D * D), w0t((size_t)D * D);
            const double scale = 1.0 / std::sqrt((double)D);
            for (int k = 0; k < D; ++k) {
                double acc = 0.0;
                for (int j = 0; j < D; ++j) acc += (double)q[j] * (double)wkv[(size_t)j * D + k];
                u[k] = (float)(acc * scale);
            }
            for (int j = 0; j < D; ++j)
                for (int k = 0; k < D; ++k) {
                    wvt[(size_t)k * D + j] = wkv[(size_t)(D + j) * D + k];
                    w0t[(size_t)k * D + j] = w0[(size_t)j * D + k];
                }
            AttnProbeW& w = m->attn_probes[layer];
            a.f32(w.u, u); a.f32(w.wvt, wvt); a.f32(w.bv, bkv.data() + D, D);
            a.f32(w.w0t, w0t); a.f32(w.b0, P(pre + "classification.0.bias"));
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

// What a step runs on: the launch sequence of a step is enqueued / captured for either half-batch chain by the same code, on the same
// weights, with the chain's own workspace and step state.  cus: the CU count its persistent GEMM grids are sized for (halved for both
// chains of a large GEMM-path batch, chain_gemm_cus); ee_fork: early-exit heads / probes may fork onto the context's side stream (not
// while `side` carries the second chain).
struct Chain {
    const WsPtrs* ws;
    StepState* st;
    int cus;
    bool ee_fork;
};
Chain whole_batch(dd_ctx* c, dd_model* m) { return Chain{&m->ws[0], c->st[0], c->num_cus, true}; }

// A loop's known region as a step sees it: the context's staged known image and mask at the step's first image, and the device rows
// (all null: none)
struct Known {
    const float* x0 = nullptr;
    const float* mask = nullptr;
    const KnownRow* ktab = nullptr;
    Known at(int b0, const dd_model* m) const {      // a chain's share: images [b0, ...)
        if (!x0) return *this;
        const size_t hw = (size_t)m->cfg.img_size * m->cfg.img_size;
        return Known{x0 + (size_t)b0 * hw * m->cfg.in_chans, mask + (size_t)b0 * hw, ktab};
    }
};

// What modifies a sampling loop, from its public entry down to the output head of each step
struct Mods {
    const dd_guidance* g = nullptr;           // classifier-free guidance: B images run as the 2 B backbone rows [x | x] with labels [y | null]
    const dd_autoguidance* ag = nullptr;      // autoguidance (never with g): a step of a model other than ag->guide runs the guide on the same rows first
    const dd_known_region* kr = nullptr;      // a *_region entry's known region as the caller passed it,
    bool region = false;                      //   which such an entry requires;
    Known kn{};                               //   staged on the device (stage_known) -- in a Slice, the chain's share of it
    const char* missing = nullptr;            // a _guided / _autoguided entry called without its struct: the rejection
    const dd_x0_threshold* thr = nullptr;     // dd_sample_multistep_threshold's thresholding as the caller passed it,
    bool thresholded = false;                 //   which that entry requires
    const dd_pag* pag = nullptr;              // perturbed-attention guidance (never with g, ag, kr or thr): B images run as the 2 B backbone rows [x | x]
    const dd_model* pag_late = nullptr;       //   with the labels [y | y]; the second half's attention is the identity in the running model's masked
                                              //   blocks: layers_late where that model is pag_late, else layers_first
    unsigned pag_mask(const dd_model* m) const { return !pag ? 0u : (pag_late && m == pag_late) ? pag->layers_late : pag->layers_first; }
};
Mods guided(const dd_guidance* g) { return Mods{.g = g, .missing = g ? nullptr : "null dd_guidance"}; }
Mods perturbed(const dd_pag* p, const dd_model* late) {
    Mods mo{};
    mo.pag = p; mo.pag_late = late; mo.missing = p ? nullptr : "null dd_pag";
    return mo;
}
Mods autoguided(const dd_autoguidance* ag) { return Mods{.ag = ag, .missing = ag ? nullptr : "null dd_autoguidance"}; }
Mods in_region(const dd_guidance* g, const dd_autoguidance* ag, const dd_known_region* kr) { return Mods{.g = g, .ag = ag, .kr = kr, .region = true}; }
Mods thresholding(const dd_guidance* g, const dd_autoguidance* ag, const dd_known_region* kr, const dd_x0_threshold* thr) {
    return Mods{.g = g, .ag = ag, .kr = kr, .region = kr != nullptr, .thr = thr, .thresholded = true};
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

// the output head's arguments that the model and the chain determine, for B images whose decoder rows are in dec; a call site sets the rest by name
FinalArgs final_args(const dd_model* m, const Chain& ch, const float* dec, const float* wconv, const float* bconv, int B) {
    FinalArgs fa{};
    fa.dec = dec; fa.wconv = wconv; fa.bconv = bconv;
    fa.st = ch.st; fa.coef = m->ctx->coef;
    fa.B = B; fa.C = m->cfg.in_chans; fa.S = m->cfg.img_size; fa.P = m->cfg.patch_size; fa.L = m->L; fa.extras = m->extras;
    return fa;
}

// ---- the forward: tokens -> blocks -> decoder_pred patches (the chain's dec) -----------------------
// early-exit taps of one forward (EarlyExitUViT.forward, early_exit.py:290-313): cls [depth, B], outs [depth, B, C, S, S]
struct EeTaps { float* cls; float* outs; int t; };

// What block bi finds already done when it starts: left by the launches in front of it (the embed launch; the previous block's last launches).
// h, frag and qkv say where its norm1 went and exclude one another; all false: the block starts from the residual stream x alone.
struct Handoff {
    bool h = false;      // its norm1 is in h (row-major)
    bool frag = false;   // the patch rows' norm1 is in hfrag, in the order the attention launch loads it: that launch computes attn.qkv (and
                         // normalises the extra-token rows itself, from x)
    bool qkv = false;    // its attn.qkv is in qkv
    bool skip = false;   // its skip_linear has run: x holds the output, ytap the block input y that its early-exit heads read
    bool xfrag = false;  // the patch rows of the residual stream are in xfrag, in the order the block tail loads them (x holds the extra-token rows only)
};

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
    float* ee_srow_all = ee_dec_all ? ee_dec_all + (size_t)nb * M * m->pd : nullptr;
    bool ao_in_frag = false;     // norm1_attention -> block_tail of the same block: the patch rows of the attention output are in aofrag

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
            HeadDecArgs ha{xin, hd.wg, hd.dc, ee_dec_all ? ee_dec_all + (size_t)bi * M * m->pd : ws.dec, M, m->pd, (L - m->extras) % 16 == 0 ? L : 0, m->extras};
            if (hd.wsplit) { ha.wg = hd.wsplit; ha.c = hd.dcs; ha.split = 1; }      // (bf16 engine: the split-bf16 product, rowops.hip SPLIT)
            if (ee_srow_all && m->ee_type != DD_EE_ATTENTION_PROBE && head_dec_probe_supported(D)) {   // ... and the MLP probe's per-token values of the same rows
                ha.srow = ee_srow_all + (size_t)bi * B * L; ha.pw_base = m->probe_w; ha.pb_base = m->probe_b; ha.st = ch.st; ha.t_mul = t_mul; ha.add = add;
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
            fa.eps_out = ee->outs + (long long)bi * B * chw;
            DD_HIP(c, launch_final(fa, hs));
        }
        if (m->ee_type == DD_EE_ATTENTION_PROBE) {
            DD_HIP(c, launch_ee_attn_probe(xin, m->attn_probes[bi], ee->cls + (long long)bi * B, B, L, D, hs));
        } else if (!probe_done) {
            if (ee_srow_all) DD_HIP(c, launch_ee_probe(xin, m->probe_w, m->probe_b, nullptr, ee_srow_all + (size_t)bi * B * L, B, L, D, ch.st, t_mul, add, hs));   // rows only: reduced behind the last block
            else DD_HIP(c, launch_ee_probe(xin, m->probe_w, m->probe_b, ee->cls + (long long)bi * B, (float*)ws.hid, B, L, D, ch.st, t_mul, add, hs));   // (the MLP hidden buffer is free between blocks)
        }
        if (side) DD_HIP(c, hipEventRecord(c->ev_ee_join, c->side));
        return DD_OK;
    }

    // out-blocks: x = skip_linear(cat[x, skip]), unless the previous block's fused launch ran it; the row-resident and split-K variants
    // leave this block's norm1 behind
    int skip_linear(int bi, Handoff& hand) {
        if (bi <= m->half_depth || hand.skip) return DD_OK;
        const BlockW& w = m->blocks[bi];
        GemmArgs<T> g{xb, skip_of(bi), (const T*)w.skip_w, w.skip_b, ws.x, nullptr, M, D, 2 * D, D, D, D, D};
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
        if (Bn > 0) DD_TIMED(DD_PROF_QKV_ATTENTION, launch_attention<T>(qkv, ao, Bn, L, m->H, D, s));
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
        T* copy = is_in ? (T*)ws.skips[bi] : (wn ? xb : nullptr);
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
            const float *ln_g = is_in ? wn->ln1_g : nullptr, *ln_b = is_in ? wn->ln1_b : nullptr;
            if (is_in && (m->rowlin_fc2 || m->splitk)) next = norm1_written();
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
        if (m->frag_skip && bi < m->half_depth) fa.out_frag = ws.skipfrags[bi];
        next.skip = m->fused_skip && bi >= m->half_depth && bi + 1 < nb;   // the next block starts with skip_linear
        if (next.skip) {
            fa.skip = (const bf16_t*)skip_of(bi + 1);
            if (m->frag_skip) fa.skip_frag = ws.skipfrags[nb - 1 - (bi + 1)];
            if (ee) fa.y_tap = ws.ytap;                                       // the next block's head / probe read y, which this launch consumes
            fa.bskip = m->blocks[bi + 1].skip_b;
        }
        // the next block's norm1 where it starts with one (behind its skip_linear, if this launch runs that); its attn.qkv inside its attention
        // launch (fused_qa), else last of all in this launch (fused_qkv) -- wherever this launch leaves that block's norm1
        const bool h_next = bi < m->half_depth || next.skip;
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

    // every layer's unpatchify + conv in one launch (layer i: images [i B, (i + 1) B) of nb B, its own conv weights), every MLP probe's mean in one
    int ee_finish() {
        if (!ee_dec_all) return DD_OK;
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

// what a forward's perturbation record is made from (Backbone::pert_first / pert_mask)
struct Perturb { int first = 0; unsigned mask = 0; };

template <typename T>
int run_backbone(dd_model* m, const Chain& ch, const float* x_img, const float* t_vec, const int64_t* y_dev, int B, hipStream_t s,
                 const EeTaps* ee = nullptr, Perturb pert = {}) {
    Backbone<T> f{m, ch, B, s, ee, pert.first, pert.mask};
    Handoff hand;
    if (int rc = f.embed(x_img, t_vec, y_dev, hand)) return rc;
    for (int bi = 0; bi < f.nb; ++bi) {
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
              const EeTaps* ee = nullptr, Perturb pert = {}) {
    return m->prec == DD_PREC_BF16 ? run_backbone<bf16_t>(m, ch, x_img, t_vec, y_dev, B, s, ee, pert)
                                   : run_backbone<float>(m, ch, x_img, t_vec, y_dev, B, s, ee, pert);
}

// the checks of a call that do not concern labels
int check_model(dd_ctx* c, dd_model* m, int B) {
    if (!c || !m) return DD_ERR_INVALID;
    if (m->ctx != c) return ctx_fail(c, DD_ERR_INVALID, "model belongs to another context");
    if (!m->finalized) return ctx_fail(c, DD_ERR_STATE, "dd_model_finalize has not been called");
    if (B < 1 || B > m->cfg.max_batch) return ctx_fail(c, DD_ERR_INVALID, "batch size outside [1, max_batch]");
    return DD_OK;
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
    return check_call(c, m, 2 * B, y_dev);
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

// The options of one model evaluation (forward_eps) or one sampling step (enqueue_step), set by name at the call site
struct StepOpts {
    const float* t_set = nullptr;      // put this timestep into the chain's step state first (else the state holds it)
    const float* t_vec = nullptr;      // per-image timesteps on the device (dd_forward*)
    const EeTaps* ee = nullptr;        // early-exit heads and probes of the forward
    Mods mods{};                       // g, ag; and (a step) kn: the known region of these B images finishes x'
    // a step only
    int noise_mode = DD_NOISE_NONE;
    const float* z = nullptr;          // DD_NOISE_BUFFER: the step's noise
    int variance = 0;
    float* eps_out = nullptr;          // the model output of the step, or null
    int advance = 0;                   // != 0: the step's last kernel also moves the device-resident timestep on (graph replays / the loops)
    const AffineRow* atab = nullptr;   // a table-driven loop: the step state holds a step index into these rows (null: the DDPM update)
    int b0 = 0;                        // first image of a half-batch chain within the whole batch
    const HistRow* htab = nullptr;     // the multistep loop (atab set): the update adds row k's history term and writes h' to h [B, C, S, S]
    float* h = nullptr;
    const X0Threshold* thr = nullptr;  // the thresholded multistep loop (htab set): the output head writes the model output to m_scratch [B, C, S, S]
    float* m_scratch = nullptr;        //   and threshold_step_kernel finishes the step
};

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
    if ((rc = run_model(m, ch, x_dev, o.t_vec, y_dev, g || pag ? 2 * B : B, s, o.ee, pert))) return rc;
    if (g) { fa.pair_B = B; fa.guide_scale = g->scale; }
    if (pag) { fa.pair_B = B; fa.guide_scale = pag->scale; }
    return DD_OK;
}

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
        ta.thr = *o.thr; ta.B = B; ta.C = m->cfg.in_chans; ta.S = m->cfg.img_size;
        DD_HIP(c, launch_threshold_step(ta, s));
        return DD_OK;
    }
    fa.x_in = x_dev; fa.z = o.z; fa.eps_out = o.eps_out; fa.x_out = x_dev;
    fa.noise_mode = o.noise_mode; fa.variance = o.variance; fa.advance = o.advance; fa.atab = o.atab; fa.b0 = o.b0;
    fa.htab = o.htab; fa.h = o.h;
    fa.kx0 = o.mods.kn.x0; fa.kmask = o.mods.kn.mask; fa.ktab = o.mods.kn.ktab;
    DD_HIP(c, launch_final(fa, s));
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

// dd_sample / dd_sample_affine with graphs: the loop runs on context-owned staging copies of x / y, so the captured step
// does not depend on the caller's tensor addresses
int grow_stage(dd_ctx* c, size_t x_elems, size_t y_elems) {
    if (int rc = c->x_stage.grow(c, x_elems)) return rc;
    return c->y_stage.grow(c, y_elems);
}
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

// dd_sample splits an even batch of at least 32 images into two half-batch chains (same-box A/B, profiles/r04/ab_chains.txt): the
// fused-path models (their kernels have strong MFMA / HBM phase structure and one tile per CU at the benchmark batch: CelebA B = 128
// +10.5 %) and GEMM-path models whose launches leave CUs idle (ImageNet-256 latents, B = 32: +9 %) as they are; GEMM-path models at
// large batches (ImageNet-64, B = 256) with the persistent GEMM grids of both chains sized for HALF the CUs (chain_gemm_cus): a full-size
// grid holds every CU's LDS, two of them only queue behind each other (-4.7 %), two half-size ones run side by side (+4.7 %).
// Development flags force the split on for any even batch, or switch it off.
bool use_chains(dd_ctx* c, dd_model* m, int B, bool early_exit_loop) {
    if ((c->dev_flags & DD_DEV_NO_CHAINS) || (B & 1) || B < 2 || ((m->ee_type >= 0) != early_exit_loop)) return false;
    return B >= 32 || (c->dev_flags & DD_DEV_FORCE_CHAINS);
}
int chain_gemm_cus(dd_ctx* c, dd_model* m, int B) {
    const bool fused = m->prec == DD_PREC_BF16 && m->fused_mlp;
    if (fused || (long long)B * m->L <= 32768) return c->num_cus;
    const int half = c->num_cus / 2 / 8 * 8;
    return half >= 8 ? half : c->num_cus;
}
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
// a failure between the fork and the join of a chained call must not leave the side stream running on the second chain's buffers behind
// the caller's back: armed after the fork, disarmed by the regular join
struct SideJoin {
    dd_ctx* c; bool armed;
    ~SideJoin() { if (armed && c->side) (void)hipStreamSynchronize(c->side); }
};

// the model's captured step of this kind for this chain and key: reused, or captured now from enqueue()
template <typename F>
int get_graph(dd_ctx* c, dd_model* m, GraphKind kind, int chain, const GraphKey& key, hipStream_t s, F&& enqueue) {
    hipGraphExec_t& exec = m->graph[kind][chain];
    if (exec && m->gkey[kind][chain] == key) return DD_OK;
    if (exec) { (void)hipGraphExecDestroy(exec); exec = nullptr; }
    hipGraph_t g = nullptr;
    DD_HIP(c, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    const int r = enqueue();
    const hipError_t e2 = hipStreamEndCapture(s, &g);
    if (r) { if (g) (void)hipGraphDestroy(g); return r; }
    if (e2 != hipSuccess) return fail_hip(c, e2, "hipStreamEndCapture");
    const hipError_t e3 = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e3 != hipSuccess) { exec = nullptr; return fail_hip(c, e3, "hipGraphInstantiate"); }
    m->gkey[kind][chain] = key;
    ++c->graph_captures;
    return DD_OK;
}

// One chain's share of a sampling loop's batch: the caller's images [b0, b0 + B), at x / y in the buffers the loop runs on
// (mods: the loop's, with the chain's share of the known region)
struct Slice { int chain, chains; float* x; const int64_t* y; int B, b0; Mods mods; };

// A sampling loop as run_loop drives it: the entry point has run its checks and supplies what differs between the loops
struct Loop {
    GraphKind kind;
    dd_model* first;
    dd_model* late;      // the model the loop may switch to (its graphs are captured along with first's), or null
    int steps;
    int switch_at;       // late runs steps [switch_at, steps), ev[1] is recorded in front of step switch_at; -1: ev[1] behind the join and the tail
    float* x_dev;
    const int64_t* y_dev;
    int B;
    Mods mods;           // (the early-exit loop: none)
    bool use_graph;
    std::function<hipError_t(StepState*, hipStream_t)> set_state;                   // a chain's step state at the start of the loop
    std::function<void(GraphKey&, const Slice&)> key;                                // the loop's own fields of a chain's graph key
    std::function<int(dd_model*, const Chain&, const Slice&, hipStream_t)> step;     // one step of one chain
    std::function<int(int chains, hipStream_t)> tail = nullptr;                      // behind the join of the chains
};

// dd_sample, dd_sample_affine (both also guided) and dd_sample_early_exit: staging, the half-batch chains, graph capture and replay, timing
int run_loop(dd_ctx* c, const Loop& L, hipStream_t s) {
    const dd_guidance* g = L.mods.g;
    const dd_autoguidance* ag = L.mods.ag;
    // Two half-batch chains (graph replays only).  Images are independent and a row's path through the kernels does not depend on the
    // batch size, so chain 0 = images [0, B0) on the caller's stream and chain 1 = images [B0, B) on the context's side stream compute
    // bit for bit what the undivided batch computes (Philox pixel ids carry the image offset) -- with the two chains free to drift apart,
    // so that one's HBM-bound phases (row prologues / epilogues, attention row fetch) run under the other's MFMA phases.
    // Guided: the decisions are made on the 2 B backbone rows and the split is by image (chain 0 takes the larger half, on the workspace
    // sized for max_batch >= 2 B rows; the second chain's workspace holds (max_batch + 1) / 2 rows >= 2 * floor(B / 2)).
    const bool ee = L.kind == GRAPH_EARLY_EXIT;
    const dd_pag* pag = L.mods.pag;
    const bool paired = g || pag;        // B images as 2 B backbone rows (stage_guided's layout): classifier-free or perturbed-attention guidance
    const int rows = paired ? 2 * L.B : L.B;
    const bool chained = L.use_graph && use_chains(c, L.first, rows, ee) && (!L.late || use_chains(c, L.late, rows, ee)) && (!paired || L.B >= 2);
    const int chains = chained ? 2 : 1;
    const int B0 = chained ? (paired ? (L.B + 1) / 2 : L.B / 2) : L.B;
    c->last_chains = chains;
    // the captured persistent GEMM grids: halved for both chains of a large GEMM-path batch (the early-exit loop keeps the full grids)
    int cus = chained && !ee ? std::min(chain_gemm_cus(c, L.first, rows), L.late ? chain_gemm_cus(c, L.late, rows) : c->num_cus) : c->num_cus;
    if (chained && ag) cus = std::min(cus, chain_gemm_cus(c, ag->guide, rows));
    // the loop runs on x_run / y_run: guided, or with graphs, the context's staging buffers (copied in here, copied back at the end)
    const size_t chw = (size_t)L.first->cfg.in_chans * L.first->cfg.img_size * L.first->cfg.img_size;
    float* x_run = L.x_dev;
    const int64_t* y_run = L.y_dev;
    int rc = DD_OK;
    if (paired) rc = stage_guided(c, L.x_dev, L.y_dev, L.B, B0, chw, g ? g->null_label : -1, s, &x_run, &y_run);
    else if (L.use_graph) rc = stage_inputs(c, L.x_dev, L.y_dev, L.B, (size_t)L.B * chw, s, &x_run, &y_run);
    if (rc) return rc;
    auto slice = [&](int k) {
        const size_t row = k ? (paired ? 2 * (size_t)B0 : (size_t)B0) : 0;     // the chain's first row in x_run / y_run
        Slice sl{k, chains, x_run + row * chw, y_run ? y_run + row : nullptr, k ? L.B - B0 : B0, k ? B0 : 0, L.mods};
        sl.mods.kn = L.mods.kn.at(sl.b0, L.first);
        return sl;
    };
    auto chain = [&](dd_model* m, int k) { return Chain{&m->ws[k], c->st[k], cus, !chained}; };
    if (L.use_graph) {
        for (int k = 0; k < chains; ++k) {
            const Slice sl = slice(k);
            GraphKey key{sl.x, sl.y, sl.B, 0, 0, cus, nullptr};
            key.b0 = sl.b0;
            key.guide(g);
            key.perturb(pag);
            key.kx0 = sl.mods.kn.x0; key.kmask = sl.mods.kn.mask; key.ktab = sl.mods.kn.ktab;
            L.key(key, sl);
            for (dd_model* m : {L.first, L.late}) {
                if (!m) continue;
                if (k && (rc = ensure_chain_ws(c, m, s))) return rc;
                GraphKey mkey = key;
                if (ag) {   // the step of the guide model itself is the unguided loop's step, under the unguided loop's key
                    if (m->cfg.num_classes <= 0) mkey.y = nullptr;
                    if (m != ag->guide) {
                        if (k && (rc = ensure_chain_ws(c, ag->guide, s))) return rc;
                        mkey.aguide = ag->guide; mkey.aserial = ag->guide->serial; mkey.gscale = __builtin_bit_cast(unsigned, ag->scale);
                    }
                }
                if ((rc = get_graph(c, m, L.kind, k, mkey, s, [&] { return L.step(m, chain(m, k), sl, s); }))) return rc;
            }
        }
    }
    for (int k = 0; k < chains; ++k) DD_HIP(c, L.set_state(c->st[k], s));
    if (chained) {
        DD_HIP(c, hipEventRecord(c->ev_fork, s));                 // the side stream starts behind the staging copies and the state
        DD_HIP(c, hipStreamWaitEvent(c->side, c->ev_fork, 0));
    }
    SideJoin side_join{c, chained};
    DD_HIP(c, hipEventRecord(c->ev[0], s));
    dd_model* cur = L.first;
    for (int k = 0; k < L.steps; ++k) {
        if (k == L.switch_at) {
            cur = L.late;
            DD_HIP(c, hipEventRecord(c->ev[1], s));
        }
        if (L.use_graph) {
            DD_HIP(c, hipGraphLaunch(cur->graph[L.kind][0], s));
            if (chained) DD_HIP(c, hipGraphLaunch(cur->graph[L.kind][1], c->side));
        } else if ((rc = L.step(cur, chain(cur, 0), slice(0), s))) {
            return rc;
        }
    }
    if (L.switch_at == L.steps) DD_HIP(c, hipEventRecord(c->ev[1], s));
    if (chained) {
        DD_HIP(c, hipEventRecord(c->ev_join, c->side));
        DD_HIP(c, hipStreamWaitEvent(s, c->ev_join, 0));
        side_join.armed = false;
    }
    if (L.tail && (rc = L.tail(chains, s))) return rc;
    if (L.switch_at < 0) DD_HIP(c, hipEventRecord(c->ev[1], s));
    DD_HIP(c, hipEventRecord(c->ev[2], s));
    if (paired) return unstage_guided(c, L.x_dev, x_run, L.B, B0, chw, s);
    if (x_run != L.x_dev) DD_HIP(c, hipMemcpyAsync(L.x_dev, x_run, (size_t)L.B * chw * sizeof(float), hipMemcpyDeviceToDevice, s));
    return DD_OK;
}

// dd_sample_early_exit's scratch for B images: eps | cls | outs.  Linear in B: chain 1's block starts behind chain 0's B0 images.
size_t ee_scratch_elems(const dd_model* m, int B) {
    const size_t chw = (size_t)m->cfg.in_chans * m->cfg.img_size * m->cfg.img_size;
    return (size_t)B * ((1 + m->cfg.depth) * chw + m->cfg.depth);
}

// dd_profile_steps (chains == 1) and dd_profile_steps_chained (chains == 2: dd_sample's two half-batch chains enqueued eagerly on `stream`
// and on the context's side stream, step by step -- the launches overlap the other chain's kernels exactly as the graph replays of the
// timed loop do): an event pair around every launch of the selected kind in every chain; out: the average ms of one such launch
int profile_steps(dd_ctx* c, dd_model* m, float* x_dev, const int64_t* y_dev, int t_start, int steps, int B, int chains, void* stream,
                  float* ms_out, int* launches_out) {
    int rc = check_call(c, m, B, y_dev);
    if (rc) return rc;
    const bool chained = chains == 2;
    if (!x_dev || !ms_out || steps < 1 || t_start > 999 || t_start - steps + 1 < 0 || (chained && ((B & 1) || B < 2)))
        return ctx_fail(c, DD_ERR_INVALID, "bad arguments");
    hipStream_t s = (hipStream_t)stream;
    const hipStream_t cs[2] = {s, c->side};
    if (chained && (rc = ensure_chain_ws(c, m, s))) return rc;
    const int B0 = B / chains;
    const size_t chw = (size_t)m->cfg.in_chans * m->cfg.img_size * m->cfg.img_size;
    const int cus = chained ? chain_gemm_cus(c, m, B) : c->num_cus;     // (both chains' persistent GEMM grids sized as dd_sample sizes them)
    if (chained) {
        DD_HIP(c, hipEventRecord(c->ev_fork, s));
        DD_HIP(c, hipStreamWaitEvent(c->side, c->ev_fork, 0));
    }
    SideJoin side_join{c, chained};
    m->time_fc1 = true;
    m->fc1_used = 0;
    for (int i = 0; i < steps && !rc; ++i) {
        hipError_t e = hipSuccess;
        for (int k = 0; k < chains && e == hipSuccess; ++k) e = launch_set_state(c->st[k], t_start - i, 12345ull, cs[k]);
        if (e != hipSuccess) { m->time_fc1 = false; return fail_hip(c, e, "set_state"); }
        for (int k = 0; k < chains && !rc; ++k) {
            const int b0 = k ? B0 : 0;
            rc = enqueue_step(c, m, Chain{&m->ws[k], c->st[k], cus, !chained}, x_dev + (size_t)b0 * chw, y_dev ? y_dev + b0 : nullptr,
                              k ? B - B0 : B0, cs[k], {.noise_mode = DD_NOISE_PHILOX, .variance = DD_VAR_BETA_TILDE, .b0 = b0});
        }
    }
    m->time_fc1 = false;
    if (rc) return rc;
    if (chained) {
        DD_HIP(c, hipEventRecord(c->ev_join, c->side));
        DD_HIP(c, hipStreamWaitEvent(s, c->ev_join, 0));
        side_join.armed = false;
    }
    DD_HIP(c, hipStreamSynchronize(s));
    double total = 0.0;
    for (size_t i = 0; i + 1 < m->fc1_used; i += 2) {
        float ms = 0.f;
        DD_HIP(c, hipEventElapsedTime(&ms, m->fc1_events[i], m->fc1_events[i + 1]));
        total += ms;
    }
    const int n = (int)(m->fc1_used / 2);
    *ms_out = n ? (float)(total / n) : 0.f;
    if (launches_out) *launches_out = n;
    return DD_OK;
}

}  // namespace

// ==========================================================================================
extern "C" {

int dd_abi_version(void) { return DD_ABI_VERSION; }

#ifndef DD_BUILD_ID
#define DD_BUILD_ID "unknown"
#endif
const char* dd_build_id(void) { return DD_BUILD_ID; }

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

int dd_ctx_create(int device, dd_ctx** out) {
    if (!out) return DD_ERR_INVALID;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return DD_ERR_HIP;
    if (hipSetDevice(device) != hipSuccess) return DD_ERR_HIP;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return DD_ERR_HIP;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return DD_ERR_UNSUPPORTED;  // gfx950 code objects only
    dd_ctx* c = new (std::nothrow) dd_ctx();
    if (!c) return DD_ERR_NOMEM;
    c->device = device;
    c->num_cus = device_num_cus();
    const Schedule& s = schedule();
    for (int i = 0; i < 1000; ++i) c->coef_host[i] = StepCoef{s.c1[i], s.c2[i], s.sigma[i], s.sigma_beta[i]};
    bool ok = hipMalloc(&c->st[0], sizeof(StepState)) == hipSuccess && hipMalloc(&c->coef, sizeof(StepCoef) * 1000) == hipSuccess &&
              hipMemcpy(c->coef, c->coef_host, sizeof(StepCoef) * 1000, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemset(c->st[0], 0, sizeof(StepState)) == hipSuccess && hipMalloc(&c->st[1], sizeof(StepState)) == hipSuccess &&
              hipMemset(c->st[1], 0, sizeof(StepState)) == hipSuccess &&
              hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking) == hipSuccess &&
              hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&c->ev_ee_fork, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&c->ev_ee_join, hipEventDisableTiming) == hipSuccess;
    for (int i = 0; ok && i < 3; ++i) ok = hipEventCreate(&c->ev[i]) == hipSuccess;
    ok = ok && hipStreamSynchronize(nullptr) == hipSuccess;     // the null-stream memsets above, before any caller stream touches the state
    ok = ok && init_gemm_kernels() == hipSuccess && init_attention_kernels() == hipSuccess &&
         init_rowops_kernels() == hipSuccess && init_mlp_fused_kernels() == hipSuccess && init_rowlin_kernels() == hipSuccess;
    if (!ok) { dd_ctx_destroy(c); return DD_ERR_HIP; }
    *out = c;
    return DD_OK;
}

void dd_ctx_destroy(dd_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->side) { (void)hipStreamSynchronize(c->side); (void)hipStreamDestroy(c->side); }
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->ev_ee_fork) (void)hipEventDestroy(c->ev_ee_fork);
    if (c->ev_ee_join) (void)hipEventDestroy(c->ev_ee_join);
    for (StepState* st : c->st) if (st) (void)hipFree(st);
    if (c->coef) (void)hipFree(c->coef);
    c->x_stage.release(); c->y_stage.release(); c->h_stage.release(); c->k_stage.release(); c->m_stage.release();
    c->atab.release(); c->htab.release(); c->ktab.release();
    for (auto& e : c->ev) if (e) (void)hipEventDestroy(e);
    delete c;
}

const char* dd_last_error(dd_ctx* c) { return c ? c->err.c_str() : "null context"; }

int dd_sync(dd_ctx* c, void* stream) {
    if (!c) return DD_ERR_INVALID;
    DD_HIP(c, hipStreamSynchronize((hipStream_t)stream));
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
    if (m->L > 288) { delete m; return ctx_fail(c, DD_ERR_UNSUPPORTED, "sequence length must be <= 288 tokens"); }
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
    if (m->warena) (void)hipFree(m->warena);
    for (char* a : m->wsarena) if (a) (void)hipFree(a);
    delete m;
}

int dd_forward(dd_ctx* c, dd_model* m, const float* x_dev, float t, const float* t_dev, const int64_t* y_dev,
               float* eps_dev, int B, void* stream) {
    int rc = check_call(c, m, B, y_dev);
    if (rc) return rc;
    if (!x_dev || !eps_dev) return ctx_fail(c, DD_ERR_INVALID, "null tensor");
    return forward_eps(c, m, whole_batch(c, m), x_dev, y_dev, eps_dev, B, (hipStream_t)stream, {.t_set = &t, .t_vec = t_dev});
}

int dd_model_enable_early_exit(dd_model* m, int classifier_type) {
    if (!m) return DD_ERR_INVALID;
    dd_ctx* c = m->ctx;
    const bool any_set = std::any_of(m->params.begin(), m->params.end(), [](const auto& kv) { return kv.second.set; });
    if (m->finalized || any_set) return ctx_fail(c, DD_ERR_STATE, "enable early exit before any parameter is set");
    if (classifier_type < DD_EE_MLP_PER_LAYER || classifier_type > DD_EE_ATTENTION_PROBE)
        return ctx_fail(c, DD_ERR_UNSUPPORTED, "unknown classifier type");
    m->ee_type = classifier_type;
    m->params = catalogue(m);   // the heads and probes of this classifier type
    return DD_OK;
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

int dd_early_exit_select(dd_ctx* c, const float* outputs_dev, const float* eps_dev, const float* classifier_dev,
                         float threshold, int depth, int B, int64_t chw, float* model_output_dev, int32_t* indices_dev,
                         float* err_mean_dev, void* stream) {
    if (!c) return DD_ERR_INVALID;
    if (!outputs_dev || !eps_dev || !classifier_dev || !model_output_dev) return ctx_fail(c, DD_ERR_INVALID, "null tensor");
    if (depth < 1 || B < 1 || chw < 1) return ctx_fail(c, DD_ERR_INVALID, "depth, B and chw must be positive");
    DD_HIP(c, launch_ee_select(outputs_dev, eps_dev, classifier_dev, threshold, depth, B, (long long)chw, model_output_dev,
                               indices_dev, err_mean_dev, (hipStream_t)stream));
    return DD_OK;
}

int dd_ddpm_step(dd_ctx* c, const float* x_dev, const float* eps_dev, const float* z_dev, int t, int variance,
                 float* x_out_dev, int64_t n, void* stream) {
    if (!c) return DD_ERR_INVALID;
    if (!x_dev || !eps_dev || !x_out_dev || n < 0) return ctx_fail(c, DD_ERR_INVALID, "null tensor");
    if (t < 0 || t > 999) return ctx_fail(c, DD_ERR_INVALID, "timestep outside [0, 999]");
    StepCoef cf = c->coef_host[t];
    if (variance == DD_VAR_BETA) cf.sigma_tilde = cf.sigma_beta;
    const int use_noise = (t > 0 && z_dev) ? 1 : 0;
    if (n == 0) return DD_OK;
    DD_HIP(c, launch_ddpm_step(x_dev, eps_dev, z_dev, x_out_dev, cf, use_noise, (long long)n, (hipStream_t)stream));
    return DD_OK;
}

int dd_ddpm_step_coef(dd_ctx* c, const float* x_dev, const float* eps_dev, const float* z_dev, float c1, float c2,
                      float sigma, float* x_out_dev, int64_t n, void* stream) {
    if (!c) return DD_ERR_INVALID;
    if (!x_dev || !eps_dev || !x_out_dev || n < 0) return ctx_fail(c, DD_ERR_INVALID, "null tensor");
    if (n == 0) return DD_OK;
    const StepCoef cf{c1, c2, sigma, sigma};
    DD_HIP(c, launch_ddpm_step(x_dev, eps_dev, z_dev, x_out_dev, cf, z_dev ? 1 : 0, (long long)n, (hipStream_t)stream));
    return DD_OK;
}

int dd_affine_step(dd_ctx* c, const float* x_dev, const float* m_dev, const float* z_dev, float a, float b, float cc,
                   float* out_dev, int64_t n, void* stream) {
    if (!c) return DD_ERR_INVALID;
    if (!x_dev || !m_dev || !out_dev || n < 0) return ctx_fail(c, DD_ERR_INVALID, "null tensor");
    if (n == 0) return DD_OK;
    DD_HIP(c, launch_affine_step(x_dev, m_dev, z_dev, out_dev, a, b, cc, (long long)n, (hipStream_t)stream));
    return DD_OK;
}

int dd_multistep_step(dd_ctx* c, const float* x_dev, const float* m_dev, const float* z_dev, float* h_dev, float a, float b, float cc,
                      float d, float p, float q, int use_hist, float* out_dev, int64_t n, void* stream) {
    if (!c) return DD_ERR_INVALID;
    if (!x_dev || !m_dev || !h_dev || !out_dev || n < 0) return ctx_fail(c, DD_ERR_INVALID, "null tensor");
    if (h_dev == x_dev || h_dev == out_dev || h_dev == m_dev) return ctx_fail(c, DD_ERR_INVALID, "h_dev must not alias x, m or out");
    if (n == 0) return DD_OK;
    DD_HIP(c, launch_multistep_step(x_dev, m_dev, z_dev, h_dev, out_dev, a, b, cc, d, p, q, use_hist ? 1 : 0, (long long)n, (hipStream_t)stream));
    return DD_OK;
}

int dd_threshold_step(dd_ctx* c, const float* x_dev, const float* m_dev, const float* z_dev, float* h_dev, const dd_x0_threshold* thr, float a,
                      float b, float cc, float d, float p, float q, int use_hist, float* out_dev, int B, int C, int S, void* stream) {
    if (!c) return DD_ERR_INVALID;
    if (!x_dev || !m_dev || !h_dev || !out_dev) return ctx_fail(c, DD_ERR_INVALID, "null tensor");
    if (h_dev == x_dev || h_dev == out_dev || h_dev == m_dev) return ctx_fail(c, DD_ERR_INVALID, "h_dev must not alias x, m or out");
    if (const char* bad = check_threshold(thr)) return ctx_fail(c, DD_ERR_INVALID, bad);
    if (B < 0 || C < 1 || S < 1) return ctx_fail(c, DD_ERR_INVALID, "bad image shape");
    const long long n = (long long)C * S * S;
    if (n > THRESHOLD_MAX_ELEMS) return ctx_fail(c, DD_ERR_UNSUPPORTED, "x0 thresholding holds one image in LDS: at most 16384 elements per image");
    if (B == 0) return DD_OK;
    ThresholdArgs ta{x_dev, m_dev, z_dev, h_dev, out_dev};
    ta.row = AffineRow{0.f, a, b, cc, z_dev ? 1 : 0, 0, 0, 0};
    ta.hr = HistRow{d, p, q, use_hist ? 1 : 0};
    ta.thr = kernel_threshold(thr, n); ta.B = B; ta.C = C; ta.S = S;
    DD_HIP(c, launch_threshold_step(ta, (hipStream_t)stream));
    return DD_OK;
}

int dd_known_blend(dd_ctx* c, const float* x_dev, const float* x0_dev, const float* mask_dev, const float* z2_dev, float ka, float kb,
                   float* out_dev, int B, int C, int S, void* stream) {
    if (!c) return DD_ERR_INVALID;
    if (!x_dev || !x0_dev || !mask_dev || !out_dev) return ctx_fail(c, DD_ERR_INVALID, "null tensor");
    if (B < 0 || C < 1 || S < 1) return ctx_fail(c, DD_ERR_INVALID, "bad image shape");
    if (B == 0) return DD_OK;
    DD_HIP(c, launch_known_blend(x_dev, x0_dev, mask_dev, z2_dev, ka, kb, out_dev, B, C, S, (hipStream_t)stream));
    return DD_OK;
}

int dd_to_images(dd_ctx* c, const float* x_dev, float* images_dev, int B, int C, int S, void* stream) {
    if (!c) return DD_ERR_INVALID;
    if (!x_dev || !images_dev) return ctx_fail(c, DD_ERR_INVALID, "null tensor");
    if (B < 0 || C < 1 || S < 1) return ctx_fail(c, DD_ERR_INVALID, "bad image shape");
    if (B == 0) return DD_OK;
    DD_HIP(c, launch_to_images(x_dev, images_dev, B, C, S, (hipStream_t)stream));
    return DD_OK;
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
    hipStream_t s = (hipStream_t)stream;
    DD_HIP(c, launch_set_state(c->st[0], t, (unsigned long long)seed, s));
    return enqueue_step(c, m, whole_batch(c, m), x_dev, y_dev, B, s,
                        {.noise_mode = noise_mode, .z = z_dev, .variance = variance, .eps_out = eps_out_dev});
}

}  // extern "C"

namespace {
// Every check the model-driven loops share, before anything is enqueued and in this order (a: any of their argument structs): the entry's
// own struct, the known region (include/duodiff.h dd_known_region), the loop's exclusion of early-exit models (no_early_exit: the
// rejection, or null), the models under the guidance in use, the loop's own arguments (own_checks), the noise mode (host_noise: the
// rejection of a host noise mode) and the image shape of the two models
template <typename Args, typename Own>
int check_loop(dd_ctx* c, const Args* a, const Mods& mo, const char* no_early_exit, const char* host_noise, Own&& own_checks) {
    if (c && mo.missing) return ctx_fail(c, DD_ERR_INVALID, mo.missing);
    if (!c || !a) return DD_ERR_INVALID;
    const dd_known_region* kr = mo.kr;
    if (mo.region) {
        if (!kr) return ctx_fail(c, DD_ERR_INVALID, "null dd_known_region");
        if (!kr->x0_dev || !kr->mask_dev || !kr->ka || !kr->kb) return ctx_fail(c, DD_ERR_INVALID, "null member of dd_known_region");
        if (mo.g && mo.ag) return ctx_fail(c, DD_ERR_INVALID, "classifier-free guidance and autoguidance are exclusive");
        if (a->noise_mode == DD_NOISE_BUFFER)
            return ctx_fail(c, DD_ERR_INVALID, "a known region draws its noise on the device; for host noise drive dd_forward, the step and dd_known_blend");
        for (dd_model* m : {a->first, a->late})
            if (m && m->ctx == c && m->ee_type >= 0) return ctx_fail(c, DD_ERR_INVALID, "a known region is not supported for early-exit models");
    }
    for (dd_model* m : {a->first, a->late})
        if (no_early_exit && m && m->ee_type >= 0) return ctx_fail(c, DD_ERR_INVALID, no_early_exit);
    if (mo.pag && a->first && a->late == a->first && mo.pag->layers_first != mo.pag->layers_late)
        return ctx_fail(c, DD_ERR_INVALID, "first and late are one model: its two perturbed-attention masks must agree");
    auto check = [&](dd_model* m) {
        if (mo.pag) return check_perturbed(c, m, a->B, a->y_dev, mo.pag, m && m == a->late ? mo.pag->layers_late : mo.pag->layers_first);
        return mo.g ? check_guided(c, m, a->B, a->y_dev, mo.g) : check_call(c, m, a->B, a->y_dev);
    };
    int rc = mo.ag ? check_autoguided(c, a->first, a->late, a->B, a->y_dev, mo.ag) : check(a->first);
    if (rc) return rc;
    if (!mo.ag && a->late && (rc = check(a->late))) return rc;
    if ((rc = own_checks())) return rc;
    if (a->noise_mode != DD_NOISE_PHILOX && a->noise_mode != DD_NOISE_NONE) return ctx_fail(c, DD_ERR_INVALID, host_noise);
    if (a->late) {
        const dd_config &f = a->first->cfg, &l = a->late->cfg;
        if (f.img_size != l.img_size || f.in_chans != l.in_chans) return ctx_fail(c, DD_ERR_INVALID, "first and late model disagree on image shape");
    }
    return DD_OK;
}
// the own checks of a table-driven loop (dd_sample_affine, dd_sample_multistep: a's fields are dd_affine_sample_args')
template <typename Args>
int check_table(dd_ctx* c, const Args* a) {
    if (!a->x_dev || !a->t || !a->a || !a->b || !a->c || !a->noise) return ctx_fail(c, DD_ERR_INVALID, "null tensor / table");
    if (a->n_steps < 1 || a->n_steps > (1 << 20)) return ctx_fail(c, DD_ERR_INVALID, "n_steps outside [1, 2^20]");
    if (a->counter_base < 0 || a->counter_base > (1 << 20)) return ctx_fail(c, DD_ERR_INVALID, "counter_base outside [0, 2^20]");
    return DD_OK;
}

// `rows` rows, row(i) each, into the table's device buffer on s.  The host copy an earlier upload may still be reading is left alone
// until that upload has finished.
template <typename Row, typename F>
int upload_rows(dd_ctx* c, RowTable<Row>& t, size_t rows, hipStream_t s, F&& row) {
    if (int rc = t.dev.grow(c, rows)) return rc;
    if (t.uploaded) DD_HIP(c, hipEventSynchronize(t.uploaded));
    else DD_HIP(c, hipEventCreateWithFlags(&t.uploaded, hipEventDisableTiming));
    t.host.resize(rows);
    for (size_t i = 0; i < rows; ++i) t.host[i] = row(i);
    DD_HIP(c, hipMemcpyAsync(t.dev.p, t.host.data(), rows * sizeof(Row), hipMemcpyHostToDevice, s));
    DD_HIP(c, hipEventRecord(t.uploaded, s));
    return DD_OK;
}
// the step table of dd_sample_affine / dd_sample_multistep on the device: n rows + one more whose timestep the last step hands on (never used)
template <typename Args>
int upload_atab(dd_ctx* c, const Args* a, hipStream_t s) {
    return upload_rows(c, c->atab, (size_t)a->n_steps + 1, s, [a](size_t k) {
        return k < (size_t)a->n_steps ? AffineRow{a->t[k], a->a[k], a->b[k], a->c[k], a->noise[k] ? 1 : 0, a->counter_base + (int)k, 0, 0}
                                      : AffineRow{0.f, 0.f, 0.f, 0.f, 0, 0, 0, 0};
    });
}

// The known region of a checked *_region call on the device (mo.kr null: nothing to do): x0 | mask copied into the context's k_stage (a
// later call with other tensors of the same shape replays the same graphs, as with x / y / h) and `rows` rows uploaded, row(i) each.
template <typename F>
int stage_known(dd_ctx* c, Mods& mo, const dd_model* m, int B, size_t rows, hipStream_t s, F&& row) {
    if (!mo.kr) return DD_OK;
    const size_t hw = (size_t)m->cfg.img_size * m->cfg.img_size, x_elems = (size_t)B * hw * m->cfg.in_chans, m_elems = (size_t)B * hw;
    if (int rc = c->k_stage.grow(c, x_elems + m_elems)) return rc;
    if (int rc = upload_rows(c, c->ktab, rows, s, row)) return rc;
    DD_HIP(c, hipMemcpyAsync(c->k_stage.p, mo.kr->x0_dev, x_elems * sizeof(float), hipMemcpyDeviceToDevice, s));
    DD_HIP(c, hipMemcpyAsync(c->k_stage.p + x_elems, mo.kr->mask_dev, m_elems * sizeof(float), hipMemcpyDeviceToDevice, s));
    mo.kn = Known{c->k_stage.p, c->k_stage.p + x_elems, c->ktab.dev.p};
    return DD_OK;
}
// ... of a table-driven loop of n steps: row k beside AffineRow k, one more (never used) as there
int stage_table_known(dd_ctx* c, Mods& mo, const dd_model* m, int B, int n, hipStream_t s) {
    const dd_known_region* kr = mo.kr;
    return stage_known(c, mo, m, B, (size_t)n + 1, s, [kr, n](size_t k) { return k < (size_t)n ? KnownRow{kr->ka[k], kr->kb[k]} : KnownRow{0.f, 0.f}; });
}

// dd_sample and its _guided, _autoguided and _region forms: one path
int sample_ddpm(dd_ctx* c, const dd_sample_args* a, Mods mo, void* stream) {
    int rc = check_loop(c, a, mo, nullptr, "dd_sample generates noise on the device; for host noise drive dd_sample_step", [&]() -> int {
        if (!a->x_dev) return ctx_fail(c, DD_ERR_INVALID, "null tensor");
        if (a->t_start > 999 || a->t_end < 0 || a->t_end > a->t_start) return ctx_fail(c, DD_ERR_INVALID, "need 999 >= t_start >= t_end >= 0");
        return DD_OK;
    });
    if (rc) return rc;
    const int n = a->t_start - a->t_end + 1;
    const bool switching = a->late && a->t_switch > 0 && a->t_switch <= 1000;
    const int t_sw = 1000 - a->t_switch;  // the late model takes over AFTER this step (sampler.py:135-136)
    const bool switch_here = switching && t_sw <= a->t_start && t_sw >= a->t_end;
    // the known rows by timestep, as the DDPM rule reads its own: row k of the call is the step at t_start - k
    auto known_row = [kr = mo.kr, t0 = a->t_start, n](size_t t) {
        const long long k = t0 - (long long)t;
        return k >= 0 && k < n ? KnownRow{kr->ka[k], kr->kb[k]} : KnownRow{0.f, 0.f};
    };
    if ((rc = stage_known(c, mo, a->first, a->B, 1000, (hipStream_t)stream, known_row))) return rc;
    Loop L{GRAPH_DDPM, a->first, switching ? a->late : nullptr, n, switch_here ? a->t_start - t_sw + 1 : -1, a->x_dev, a->y_dev, a->B, mo,
           a->use_graph != 0};
    L.set_state = [&](StepState* st, hipStream_t s) { return launch_set_state(st, a->t_start, (unsigned long long)a->seed, s); };
    L.key = [&](GraphKey& k, const Slice&) { k.noise = a->noise_mode; k.variance = a->variance; };
    L.step = [&](dd_model* m, const Chain& ch, const Slice& sl, hipStream_t s) {
        return enqueue_step(c, m, ch, sl.x, sl.y, sl.B, s,
                            {.mods = sl.mods, .noise_mode = a->noise_mode, .variance = a->variance, .advance = 1, .b0 = sl.b0});
    };
    return run_loop(c, L, (hipStream_t)stream);
}

// dd_sample_affine and its _guided, _autoguided and _region forms: one path
int sample_affine(dd_ctx* c, const dd_affine_sample_args* a, Mods mo, void* stream) {
    int rc = check_loop(c, a, mo, nullptr, "dd_sample_affine generates noise on the device; for host noise drive dd_forward + dd_affine_step",
                        [&] { return check_table(c, a); });
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int n = a->n_steps;
    const bool switching = a->late && a->switch_after >= 0 && a->switch_after < n;
    if ((rc = upload_atab(c, a, s))) return rc;
    if ((rc = stage_table_known(c, mo, a->first, a->B, n, s))) return rc;
    const AffineRow* atab = c->atab.dev.p;
    // (two half-batch chains, as dd_sample: both read the one step table; each has its own step index and Philox image offset)
    Loop L{GRAPH_AFFINE, a->first, switching ? a->late : nullptr, n, switching ? a->switch_after : -1, a->x_dev, a->y_dev, a->B, mo,
           a->use_graph != 0};
    L.set_state = [&](StepState* st, hipStream_t ss) { return launch_set_state_table(st, atab, (unsigned long long)a->seed, ss); };
    L.key = [&](GraphKey& k, const Slice&) { k.noise = a->noise_mode; k.atab = atab; };
    L.step = [&](dd_model* m, const Chain& ch, const Slice& sl, hipStream_t ss) {
        return enqueue_step(c, m, ch, sl.x, sl.y, sl.B, ss, {.mods = sl.mods, .noise_mode = a->noise_mode, .advance = 1, .atab = atab, .b0 = sl.b0});
    };
    return run_loop(c, L, s);
}

// dd_sample_multistep and its forms: dd_sample_affine's loop with the history register.  h is staged like x: copied into the context's
// h_stage before the loop, chain k's images at h_stage + o_k chw (guided too: h holds B images, not 2 B), and copied back behind the
// join of the chains.
int sample_multistep(dd_ctx* c, const dd_multistep_sample_args* a, Mods mo, void* stream) {
    int rc = check_loop(c, a, mo, "the multistep loop is not supported for early-exit models",
                        "dd_sample_multistep generates noise on the device; for host noise drive dd_forward + dd_multistep_step",
                        [&] { return check_table(c, a); });
    if (rc) return rc;
    if (!a->d || !a->p || !a->q || !a->hist) return ctx_fail(c, DD_ERR_INVALID, "null tensor / table");
    if (!a->h_dev) return ctx_fail(c, DD_ERR_INVALID, "null h_dev: the multistep loop needs its history register");
    X0Threshold thr{};
    if (mo.thresholded) {
        if (const char* bad = check_threshold(mo.thr)) return ctx_fail(c, DD_ERR_INVALID, bad);
        const long long n_img = (long long)a->first->cfg.in_chans * a->first->cfg.img_size * a->first->cfg.img_size;
        if (n_img > THRESHOLD_MAX_ELEMS) return ctx_fail(c, DD_ERR_UNSUPPORTED, "x0 thresholding holds one image in LDS: at most 16384 elements per image");
        thr = kernel_threshold(mo.thr, n_img);
    }
    hipStream_t s = (hipStream_t)stream;
    const int n = a->n_steps;
    const bool switching = a->late && a->switch_after >= 0 && a->switch_after < n;
    if ((rc = upload_atab(c, a, s))) return rc;
    rc = upload_rows(c, c->htab, (size_t)n + 1, s, [a, n](size_t k) {
        return k < (size_t)n ? HistRow{a->d[k], a->p[k], a->q[k], a->hist[k] ? 1 : 0} : HistRow{0.f, 0.f, 0.f, 0};
    });
    if (rc) return rc;
    const size_t chw = (size_t)a->first->cfg.in_chans * a->first->cfg.img_size * a->first->cfg.img_size;
    const size_t h_elems = (size_t)a->B * chw;
    if ((rc = c->h_stage.grow(c, h_elems))) return rc;
    float* h_run = c->h_stage.p;
    if (mo.thresholded && (rc = c->m_stage.grow(c, h_elems))) return rc;      // (with h_stage: never on the launch path)
    float* m_run = mo.thresholded ? c->m_stage.p : nullptr;
    const X0Threshold* thr_p = mo.thresholded ? &thr : nullptr;
    DD_HIP(c, hipMemcpyAsync(h_run, a->h_dev, h_elems * sizeof(float), hipMemcpyDeviceToDevice, s));
    if ((rc = stage_table_known(c, mo, a->first, a->B, n, s))) return rc;
    const AffineRow* atab = c->atab.dev.p;
    const HistRow* htab = c->htab.dev.p;
    Loop L{GRAPH_MULTISTEP, a->first, switching ? a->late : nullptr, n, switching ? a->switch_after : -1, a->x_dev, a->y_dev, a->B, mo,
           a->use_graph != 0};
    L.set_state = [&](StepState* st, hipStream_t ss) { return launch_set_state_table(st, atab, (unsigned long long)a->seed, ss); };
    L.key = [&](GraphKey& k, const Slice&) {
        k.noise = a->noise_mode; k.atab = atab; k.aux0 = htab; k.aux1 = h_run;
        if (mo.thresholded) {
            k.tmode = mo.thr->mode; k.tscratch = m_run;
            k.tq = __builtin_bit_cast(unsigned, mo.thr->quantile); k.tr = __builtin_bit_cast(unsigned, mo.thr->range);
            k.ts = __builtin_bit_cast(unsigned, mo.thr->s_max);
        }
    };
    L.step = [&](dd_model* m, const Chain& ch, const Slice& sl, hipStream_t ss) {
        return enqueue_step(c, m, ch, sl.x, sl.y, sl.B, ss, {.mods = sl.mods, .noise_mode = a->noise_mode, .advance = 1, .atab = atab, .b0 = sl.b0,
                                                             .htab = htab, .h = h_run + (size_t)sl.b0 * chw, .thr = thr_p,
                                                             .m_scratch = m_run ? m_run + (size_t)sl.b0 * chw : nullptr});
    };
    L.tail = [&](int, hipStream_t ss) -> int {
        DD_HIP(c, hipMemcpyAsync(a->h_dev, h_run, h_elems * sizeof(float), hipMemcpyDeviceToDevice, ss));
        return DD_OK;
    };
    return run_loop(c, L, s);
}
}  // namespace

extern "C" {

int dd_sample(dd_ctx* c, const dd_sample_args* a, void* stream) { return sample_ddpm(c, a, Mods{}, stream); }
int dd_sample_guided(dd_ctx* c, const dd_sample_args* a, const dd_guidance* g, void* stream) { return sample_ddpm(c, a, guided(g), stream); }
int dd_sample_autoguided(dd_ctx* c, const dd_sample_args* a, const dd_autoguidance* g, void* stream) { return sample_ddpm(c, a, autoguided(g), stream); }
int dd_sample_region(dd_ctx* c, const dd_sample_args* a, const dd_guidance* g, const dd_autoguidance* ag, const dd_known_region* kr, void* stream) {
    return sample_ddpm(c, a, in_region(g, ag, kr), stream);
}
int dd_sample_affine(dd_ctx* c, const dd_affine_sample_args* a, void* stream) { return sample_affine(c, a, Mods{}, stream); }
int dd_sample_affine_guided(dd_ctx* c, const dd_affine_sample_args* a, const dd_guidance* g, void* stream) { return sample_affine(c, a, guided(g), stream); }
int dd_sample_affine_autoguided(dd_ctx* c, const dd_affine_sample_args* a, const dd_autoguidance* g, void* stream) {
    return sample_affine(c, a, autoguided(g), stream);
}
int dd_sample_affine_region(dd_ctx* c, const dd_affine_sample_args* a, const dd_guidance* g, const dd_autoguidance* ag, const dd_known_region* kr,
                            void* stream) {
    return sample_affine(c, a, in_region(g, ag, kr), stream);
}
int dd_sample_multistep(dd_ctx* c, const dd_multistep_sample_args* a, void* stream) { return sample_multistep(c, a, Mods{}, stream); }
int dd_sample_multistep_guided(dd_ctx* c, const dd_multistep_sample_args* a, const dd_guidance* g, void* stream) {
    return sample_multistep(c, a, guided(g), stream);
}
int dd_sample_multistep_autoguided(dd_ctx* c, const dd_multistep_sample_args* a, const dd_autoguidance* g, void* stream) {
    return sample_multistep(c, a, autoguided(g), stream);
}
int dd_sample_perturbed(dd_ctx* c, const dd_sample_args* a, const dd_pag* p, void* stream) {
    return sample_ddpm(c, a, perturbed(p, a ? a->late : nullptr), stream);
}
int dd_sample_affine_perturbed(dd_ctx* c, const dd_affine_sample_args* a, const dd_pag* p, void* stream) {
    return sample_affine(c, a, perturbed(p, a ? a->late : nullptr), stream);
}
int dd_sample_multistep_perturbed(dd_ctx* c, const dd_multistep_sample_args* a, const dd_pag* p, void* stream) {
    return sample_multistep(c, a, perturbed(p, a ? a->late : nullptr), stream);
}
int dd_sample_multistep_region(dd_ctx* c, const dd_multistep_sample_args* a, const dd_guidance* g, const dd_autoguidance* ag,
                               const dd_known_region* kr, void* stream) {
    return sample_multistep(c, a, in_region(g, ag, kr), stream);
}
int dd_sample_multistep_threshold(dd_ctx* c, const dd_multistep_sample_args* a, const dd_guidance* g, const dd_autoguidance* ag,
                                  const dd_known_region* kr, const dd_x0_threshold* thr, void* stream) {
    if (c && g && ag) return ctx_fail(c, DD_ERR_INVALID, "classifier-free guidance and autoguidance are exclusive");
    return sample_multistep(c, a, thresholding(g, ag, kr, thr), stream);
}

// One early-exit sampling step on the device (reference eesampler.py:56-81): EarlyExitUViT.forward with every head and
// probe -> per-sample exit selection -> DDPM update with the selected output; rows t of the two log tables are written.
// ws: the chain's scratch block (eps | cls | outs for B images, ee_scratch_elems); b0 / B_all: the chain's first image within the whole batch
// and the whole batch (idx_tab rows are B_all wide); sums: err_tab is the chain's table of per-layer SUMS (launch_ee_mean_combine joins the chains)
static int enqueue_ee_step(dd_ctx* c, dd_model* m, const Chain& ch, float* ws, float* x, const int64_t* y, float thr, float* err_tab,
                           int32_t* idx_tab, int noise_mode, int B, hipStream_t s, int b0, int B_all, bool sums) {
    const long long chw = (long long)m->cfg.in_chans * m->cfg.img_size * m->cfg.img_size;
    const int depth = m->cfg.depth;
    float* eps = ws;
    float* cls = eps + (size_t)B * chw;
    float* outs = cls + (size_t)depth * B;
    const EeTaps ee{cls, outs, 0};
    if (int rc = forward_eps(c, m, ch, x, y, eps, B, s, {.ee = &ee})) return rc;
    // exit layer per image, the selected output and the DDPM update in one launch (dd_early_exit_select + the step kernel, fused: same arithmetic)
    DD_HIP(c, launch_ee_select_step(x, outs, eps, cls, thr, depth, idx_tab, err_tab, B_all, b0, sums, ch.st, c->coef, B,
                                    m->cfg.in_chans, m->cfg.img_size, noise_mode, 1, s));
    return DD_OK;
}

int dd_sample_early_exit(dd_ctx* c, const dd_ee_sample_args* a, void* stream) {
    if (!c || !a) return DD_ERR_INVALID;
    dd_model* m = a->model;
    int rc = check_call(c, m, a->B, a->y_dev);
    if (rc) return rc;
    if (m->ee_type < 0) return ctx_fail(c, DD_ERR_STATE, "model was not created with dd_model_enable_early_exit");
    if (!a->x_dev) return ctx_fail(c, DD_ERR_INVALID, "null tensor");
    if (a->t_start > 999 || a->t_end < 0 || a->t_end > a->t_start) return ctx_fail(c, DD_ERR_INVALID, "need 999 >= t_start >= t_end >= 0");
    if (a->noise_mode != DD_NOISE_PHILOX && a->noise_mode != DD_NOISE_NONE)
        return ctx_fail(c, DD_ERR_INVALID, "dd_sample_early_exit generates noise on the device; for host noise drive dd_forward_early_exit");
    // Two half-batch chains, as dd_sample: the samples are independent (every exit decision is per sample); the one quantity over the whole
    // batch -- the logged per-layer mean of the predicted errors, eesampler.py:70 -- becomes per-chain sums that one small launch joins
    // behind the loop, (chain 0 + chain 1) / B.  Heads and probes stay on each chain's own stream (measured: the 13 forks as parallel
    // branches of each chain's graph cost +0.9 ms per step -- 5.22 against 4.23 ms; profiles/r05/ab_round5.txt).
    const size_t tab = (size_t)1000 * m->cfg.depth;
    if (!m->ee_ws) DD_HIP(c, hipMalloc((void**)&m->ee_ws, (ee_scratch_elems(m, m->cfg.max_batch) + 2 * tab) * sizeof(float)));
    float* sums = m->ee_ws + ee_scratch_elems(m, m->cfg.max_batch);
    auto err_tab = [&](const Slice& sl) { return sl.chains == 1 || !a->err_dev ? a->err_dev : sums + sl.chain * tab; };
    Loop L{GRAPH_EARLY_EXIT, m, nullptr, a->t_start - a->t_end + 1, -1, a->x_dev, a->y_dev, a->B, Mods{}, a->use_graph != 0};
    L.set_state = [&](StepState* st, hipStream_t s) { return launch_set_state(st, a->t_start, (unsigned long long)a->seed, s); };
    L.key = [&](GraphKey& k, const Slice& sl) {
        k.noise = a->noise_mode; k.aux0 = err_tab(sl); k.aux1 = a->idx_dev; k.thr = a->threshold;
        if (sl.chains == 2 && sl.chain == 0) k.b0 = -1;     // (chain 0 of two -- not the whole batch's graph)
    };
    L.step = [&](dd_model* mm, const Chain& ch, const Slice& sl, hipStream_t s) {
        return enqueue_ee_step(c, mm, ch, mm->ee_ws + ee_scratch_elems(mm, sl.b0), sl.x, sl.y, a->threshold, err_tab(sl), a->idx_dev,
                               a->noise_mode, sl.B, s, sl.b0, a->B, sl.chains == 2);
    };
    L.tail = [&](int chains, hipStream_t s) -> int {
        if (chains == 2 && a->err_dev) DD_HIP(c, launch_ee_mean_combine(sums, sums + tab, a->err_dev, m->cfg.depth, a->t_end, a->t_start, a->B, s));
        return DD_OK;
    };
    return run_loop(c, L, (hipStream_t)stream);
}

long long dd_dev_graph_captures(dd_ctx* c) { return c ? c->graph_captures : -1; }
int dd_dev_last_sample_chains(dd_ctx* c) { return c ? c->last_chains : -1; }

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

int dd_dev_set_flags(dd_ctx* c, unsigned flags) {
    if (!c) return DD_ERR_INVALID;
    c->dev_flags = flags;
    return DD_OK;
}

int dd_profile_select(dd_ctx* c, int kind) {
    if (!c || kind < DD_PROF_DOMINANT || kind > DD_PROF_SPLITK) return DD_ERR_INVALID;
    c->prof_kind = kind;
    return DD_OK;
}

int dd_last_sample_timing(dd_ctx* c, float out3[3]) {
    if (!c || !out3) return DD_ERR_INVALID;
    DD_HIP(c, hipEventSynchronize(c->ev[2]));
    DD_HIP(c, hipEventElapsedTime(&out3[0], c->ev[0], c->ev[2]));
    DD_HIP(c, hipEventElapsedTime(&out3[1], c->ev[0], c->ev[1]));
    DD_HIP(c, hipEventElapsedTime(&out3[2], c->ev[1], c->ev[2]));
    return DD_OK;
}

int dd_profile_steps(dd_ctx* c, dd_model* m, float* x_dev, const int64_t* y_dev, int t_start, int steps, int B,
                     void* stream, float* fc1_ms_out, int* launches_out) {
    return profile_steps(c, m, x_dev, y_dev, t_start, steps, B, 1, stream, fc1_ms_out, launches_out);
}
int dd_profile_steps_chained(dd_ctx* c, dd_model* m, float* x_dev, const int64_t* y_dev, int t_start, int steps, int B,
                             void* stream, float* ms_out, int* launches_out) {
    return profile_steps(c, m, x_dev, y_dev, t_start, steps, B, 2, stream, ms_out, launches_out);
}

int dd_bench_gemm(dd_ctx* c, dd_model* m, int B, int iters, void* stream, float* ms_out, double* flops_out) {
    int rc = check_call(c, m, B, m && m->cfg.num_classes > 0 ? (const int64_t*)1 : nullptr);
    if (rc) return rc;
    if (iters < 1 || !ms_out) return ctx_fail(c, DD_ERR_INVALID, "bad arguments");
    hipStream_t s = (hipStream_t)stream;
    const int M = B * m->L, D = m->D;
    const BlockW& w = m->blocks[0];
    auto once = [&]() -> hipError_t {
        if (m->prec == DD_PREC_BF16) {
            GemmArgs<bf16_t> g{(const bf16_t*)m->ws[0].h, nullptr, (const bf16_t*)w.fc1_w, w.fc1_b, nullptr, (bf16_t*)m->ws[0].hid,
                               M, m->hidden, D, D, D, 0, m->hid_ld};
            return launch_gemm<bf16_t>(g, EPI_BIAS_GELU, s, c->num_cus);
        }
        GemmArgs<float> g{(const float*)m->ws[0].h, nullptr, (const float*)w.fc1_w, w.fc1_b, nullptr, (float*)m->ws[0].hid,
                          M, m->hidden, D, D, D, 0, m->hid_ld};
        return launch_gemm<float>(g, EPI_BIAS_GELU, s, c->num_cus);
    };
    DD_HIP(c, once());
    DD_HIP(c, time_launches(s, iters, once, ms_out));
    if (flops_out) *flops_out = 2.0 * (double)M * (double)m->hidden * (double)D;
    return DD_OK;
}

int dd_plan_rows(int M, int N, int K, int num_cus, int* q_out, int* e_out) {
    if (!q_out || !e_out) return DD_ERR_INVALID;
    return plan_rows_256(M, N, K, num_cus, q_out, e_out) ? DD_OK : DD_ERR_UNSUPPORTED;
}

int dd_set_num_cus(dd_ctx* c, int n) {
    if (!c) return DD_ERR_INVALID;
    if (n < 8) return ctx_fail(c, DD_ERR_INVALID, "need at least 8 CUs");
    c->num_cus = n / 8 * 8;      // the persistent kernels deal tiles to workgroups in groups of 8 (one per XCD)
    return DD_OK;
}

}  // extern "C"
