// The engine's host-side state, shared by the translation units behind the C ABI (capi.hip, loops.hip, forward.hip, model.hip, and vae.hip /
// dev_harness.hip for the context's fields): the context and the model behind the opaque handles of include/duodiff.h, the records a step and a
// sampling loop are described with, and the declarations of the functions that cross a unit boundary.  The units depend one way,
// capi -> loops -> forward -> model: a lower unit never calls an upper one (ctx_fail, which every unit calls, is defined in model.hip).
// Hidden visibility for everything but the two opaque structs: nothing here joins the library's dynamic symbol table.  Host only: not included by
// any kernel translation unit, dd_internal.h or wave_prims.h.
#pragma once
#include "../../include/duodiff.h"
#include "dd_internal.h"
#include "dev_scope.h"

#include <map>
#include <string>
#include <vector>

#define DD_HIP(c, expr)                                          \
    do {                                                         \
        hipError_t _e = (expr);                                  \
        if (_e != hipSuccess) return dd::fail_hip((c), _e, #expr);   \
    } while (0)

#pragma GCC visibility push(hidden)
namespace dd {
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
// What a captured step was captured for: a graph is replayed while its key matches (in front of dd_ctx, which holds the jump's graphs)
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
    const void* seeds = nullptr;                                     // per-image seeds: the context's staged copy (null: the plain noise)
    int jchans = 0, jsize = 0;                                       // a jump's graph (dd_ctx::jump_graph: no model's): the image shape C, S
    int cblocks = 0, corder = 0;                                     // block caching: K (0: none) and the order
    bool operator==(const GraphKey&) const = default;
    void perturb(const dd_pag* p) {
        if (p) { pag = 1; gscale = __builtin_bit_cast(unsigned, p->scale); pfirst = p->layers_first; plate = p->layers_late; }
    }
    void guide(const dd_guidance* g) {
        if (g) { gnull = g->null_label; gscale = __builtin_bit_cast(unsigned, g->scale); }
    }
};

// the captured step of each sampling loop: dd_model::graph[kind][chain]
// (GRAPH_AFFINE_REUSE: the reuse step of dd_sample_affine_cached, beside the refresh step in GRAPH_AFFINE)
enum GraphKind { GRAPH_DDPM, GRAPH_AFFINE, GRAPH_EARLY_EXIT, GRAPH_MULTISTEP, GRAPH_SCAN, GRAPH_SCAN_EXITS, GRAPH_AFFINE_REUSE, GRAPH_KINDS };
}  // namespace dd
#pragma GCC visibility pop

// ------------------------------------------------------------------------------------------
struct dd_ctx {
    int device = 0;
    std::string err;
    dd::StepState* st[2] = {nullptr, nullptr};   // device: the step state (timestep / counter) of each half-batch chain (Chain)
    hipStream_t side = nullptr;  // the second chain's stream (context-owned, non-blocking)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev_ee_fork = nullptr, ev_ee_join = nullptr;   // early-exit heads / probes of a layer on the side stream, beside the block's attention launch
    dd::StepCoef* coef = nullptr;    // device [1000]
    dd::StepCoef coef_host[1000];
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    float timing[3] = {0, 0, 0};
    int num_cus = 256;           // CU count the persistent GEMM grids are sized for (dd_set_num_cus), a multiple of 8
    // dd_sample's graphs run on context-owned staging copies of x / y, so a captured step does not depend on the caller's
    // tensor addresses (reference get_samples allocates a fresh x per call: the graphs would be re-captured every time)
    dd::DevBuf<float> x_stage;
    dd::DevBuf<int64_t> y_stage;
    long long graph_captures = 0;
    int last_chains = 1;         // chains the last dd_sample call ran (dd_dev_last_sample_chains)
    hipGraphExec_t jump_graph[2] = {nullptr, nullptr};   // dd_sample_affine_walk: the captured resampling jump of each chain (launch_jump: it runs no
    dd::GraphKey jump_key[2]{};                          //   model, so it lives here), keyed like a step's graph
    dd::RowTable<dd::AffineRow> atab;    // dd_sample_affine: the step table
    dd::RowTable<dd::HistRow> htab;      // dd_sample_multistep: the history half of the rows beside atab,
    dd::DevBuf<float> h_stage;       //   and the history register the loop runs on ([B, C, S, S], staged like x)
    dd::RowTable<dd::KnownRow> ktab;     // the *_region loops: the known-region half of the rows,
    dd::DevBuf<float> k_stage;       //   and the known image and mask the loop reads (x0 [B, C, S, S] | mask [B, 1, S, S], staged like x)
    dd::DevBuf<float> m_stage;       // dd_sample_multistep_threshold: the step's (guided) model output [B, C, S, S], chain k's images at its first image:
                                 //   written by the output head and read by threshold_step_kernel within one step, never across steps
    dd::RowTable<dd::ScanRow> stab;      // the scans (loops.hip stage_scan fills both).  dd_scan_error: the scan's rows,
    dd::DevBuf<float> scan_ws;       //   and its scratch, x_t | eps ([B, C, S, S] each; chain k's images at its first image) | err [n, B]: grown before the loop,
                                 //   never on the launch path.  dd_scan_error_early_exit: x_t | mse [n, depth + 1, B] | target (the same) | pred [n, depth, B]; its
                                 //   table has 1001 rows (by timestep, and the base row) and its taps live in the model's ee_ws
    // dd_set_image_seeds: the caller's per-image seeds (device, seeds_n of them; null: the plain noise), and the context's own copy that
    // the kernels read -- copied at every call that draws device noise (stage_image_seeds), so a captured step is reused across seeds
    const uint64_t* seeds_user = nullptr;
    int seeds_n = 0;
    dd::DevBuf<unsigned long long> seeds_stage;
    long long real_stats[3] = {0, 0, 0};     // dd_sample_early_exit_real's last call: block-rows run, moves made, compactions made (dd_dev_ee_real_stats),
    double real_wait_ms = 0.0;               //   the time its calling thread spent waiting for counts and the number of such waits (dd_dev_ee_real_wait)
    long long real_waits = 0, real_bytes = 0;   //   and the bytes its compactions moved
    int prof_kind = 0;           // dd_profile_select: which launches dd_profile_steps brackets (DD_PROF_*)
    unsigned dev_flags = 0;      // dd_dev_set_flags (include/duodiff_dev.h): kernel-variant switches of the development harness
};

#pragma GCC visibility push(hidden)
namespace dd {

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

// The block cache of one chain of a model (include/duodiff.h dd_block_cache): y_deep of the last refresh, of the one before it, and the
// extrapolated y^ an order-1 reuse step reads -- [Mp, D] of the activation type each, laid out like WsPtrs::xb, allocated on first use
// (ensure_block_cache) and outside the workspace arena: no other forward writes them.  Beside them the host-side validity: what the
// buffers hold, carried across calls so that a loop cut at a save point continues where the uncut loop would.
struct BlockCache {
    void *last = nullptr, *prev = nullptr, *yhat = nullptr;
    int K = 0, rows = 0, b0 = 0, B = 0;     // the geometry `last` was written under: blocks, backbone rows, the chain's first image and size
    bool has_last = false, has_prev = false;
    bool holds(int K_, int rows_, int b0_, int B_) const { return has_last && K == K_ && rows == rows_ && b0 == b0_ && B == B_; }
    // a refresh of this geometry; rotate: prev <- last went first
    void refresh(int K_, int rows_, int b0_, int B_, bool rotate) {
        has_prev = rotate && holds(K_, rows_, b0_, B_);
        K = K_; rows = rows_; b0 = b0_; B = B_; has_last = true;
    }
};

}  // namespace dd
#pragma GCC visibility pop

struct dd_model {
    dd_ctx* ctx = nullptr;
    unsigned long long serial = 0;   // unique per dd_model_create of the process (graph keys that name another model: autoguidance)
    dd_config cfg{};
    int D = 0, L = 0, N = 0, extras = 0, pd = 0, pdp = 0, H = 0, hidden = 0, hid_ld = 0, half_depth = 0, Mp_max = 0;
    std::map<std::string, dd::HostParam> params;   // every state_dict name of the model (catalogue), its data once set (dropped by finalize)
    bool finalized = false;
    int prec = DD_PREC_BF16;
    size_t esize = 2;
    char* warena = nullptr;    // weights
    std::vector<dd::BlockW> blocks;  // in.., mid, out..
    const float *emb_wt = nullptr, *emb_b = nullptr, *pos = nullptr, *label = nullptr;
    const float *tm_w1t = nullptr, *tm_b1 = nullptr, *tm_w2t = nullptr, *tm_b2 = nullptr;   // time_embed MLP (mlp_time_embed)
    dd::HeadW head{};                         // the final head (uvit.py:377-380; no split-bf16 image)
    // early-exit baseline (models/early_exit.py:193-268): per-layer output heads + MLP probes; ee_type < 0: plain U-ViT
    int ee_type = -1, n_probe = 0;
    std::vector<dd::HeadW> heads;             // head i is applied to the input of block i
    const float *probe_w = nullptr, *probe_b = nullptr;   // [n_probe, D], [n_probe]
    std::vector<dd::AttnProbeW> attn_probes;                  // DD_EE_ATTENTION_PROBE: one per layer
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
    dd::WsPtrs ws[2];
    hipGraphExec_t graph[dd::GRAPH_KINDS][2] = {};                // each loop's captured step, per chain
    dd::GraphKey gkey[dd::GRAPH_KINDS][2]{};
    dd::BlockCache cache[2];                                 // block caching: each chain's cache (ensure_block_cache)
    float* ee_ws = nullptr;                                  // dd_sample_early_exit scratch: eps | cls | outs (two chains: one such block per chain, half the batch each),
                                                             // then the chains' per-step sums of the predicted errors [2][1000][depth]
    // dd_sample_early_exit_real: each chain's tables on the device (RealTables, one allocation), the pinned pair of counts each chain's
    // compaction layers copy to the host, and the event behind that copy
    int* real_tabs = nullptr;
    int* real_counts_host = nullptr;
    hipEvent_t real_ev[2] = {nullptr, nullptr};
    // in-context timing (dd_profile_steps): event pairs recorded around each launch of kind ctx->prof_kind when enabled
    bool time_fc1 = false;
    std::vector<hipEvent_t> fc1_events;   // pairs, grown on demand
    size_t fc1_used = 0;
};

#pragma GCC visibility push(hidden)
namespace dd {

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
    const unsigned long long* seeds = nullptr;   // per-image seeds of the WHOLE batch, staged (stage_image_seeds), or null: in a Slice too -- the
                                              //   kernels index them by b0 + b, the image, under either guidance that doubles the rows
    unsigned pag_mask(const dd_model* m) const { return !pag ? 0u : (pag_late && m == pag_late) ? pag->layers_late : pag->layers_first; }
};

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

// early-exit taps of one forward (EarlyExitUViT.forward, early_exit.py:290-313): cls [depth, B], outs [depth, B, C, S, S]
struct EeTaps { float* cls; float* outs; int t; };

// what a forward's perturbation record is made from (Backbone::pert_first / pert_mask)
struct Perturb { int first = 0; unsigned mask = 0; };

// What one forward does with the chain's block cache (BlockCache; Backbone reads it).  blocks == 0: nothing, the forward of an uncached call.
// A refresh runs every block and stores y_deep, the output of block nb - 1 - K, in `last` (rotate: prev <- last first).  A reuse skips blocks
// K .. nb - 1 - K: out-block nb - K takes y^ for its x operand -- `last` itself, or (extrapolate) what cache_extrapolate_kernel leaves in yhat:
// under atab the op and w of the table's current row (an order-1 loop's reuse step, captured once for both ops), else last + w (last - prev).
struct CacheUse {
    int blocks = 0;                    // K
    bool reuse = false;                // a reuse step (else a refresh)
    bool rotate = false;               // a refresh: prev <- last first
    bool extrapolate = false;          // a reuse: y^ comes from the kernel
    float w = 0.f;                     //   with this weight,
    const AffineRow* atab = nullptr;   //   or with the op and w of the step table's current row
};

// The options of one model evaluation (forward_eps) or one sampling step (enqueue_step), set by name at the call site
struct StepOpts {
    const float* t_set = nullptr;      // put this timestep into the chain's step state first (else the state holds it)
    const float* t_vec = nullptr;      // per-image timesteps on the device (dd_forward*)
    const EeTaps* ee = nullptr;        // early-exit heads and probes of the forward
    Mods mods{};                       // g, ag; and (a step) kn: the known region of these B images finishes x'
    CacheUse cache{};                  // block caching of this forward (none: blocks == 0)
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

// ---- model.hip
// the fp32 schedule tables of the reference's 1000-step linear schedule
struct Schedule {
    float betas[1000], alphas[1000], abar[1000], abar_prev[1000], bt_sampler[1000], bt_sched[1000];
    float c1[1000], c2[1000], sigma[1000], sigma_beta[1000];
    Schedule();
};
const Schedule& schedule();
int ensure_chain_ws(dd_ctx* c, dd_model* m, hipStream_t s);   // the second half-batch chain's workspace, laid out on the first chained call
int ensure_block_cache(dd_ctx* c, dd_model* m, int chain, hipStream_t s);   // a chain's block cache, allocated and zeroed (on s) on first use

// ---- forward.hip
Mods perturbed(const dd_pag* p, const dd_model* late);
const char* check_threshold(const dd_x0_threshold* t);
X0Threshold kernel_threshold(const dd_x0_threshold* t, long long n);
int check_call(dd_ctx* c, dd_model* m, int B, const int64_t* y_dev);
int check_guided(dd_ctx* c, dd_model* m, int B, const int64_t* y_dev, const dd_guidance* g);
int check_perturbed(dd_ctx* c, dd_model* m, int B, const int64_t* y_dev, const dd_pag* p, unsigned mask);
int check_cached(dd_ctx* c, dd_model* m, int blocks);
int check_autoguided(dd_ctx* c, dd_model* first, dd_model* late, int B, const int64_t* y_dev, const dd_autoguidance* ag);
int enqueue_step(dd_ctx* c, dd_model* m, const Chain& ch, float* x_dev, const int64_t* y_dev, int B, hipStream_t s, const StepOpts& o);
int forward_eps(dd_ctx* c, dd_model* m, const Chain& ch, const float* x_dev, const int64_t* y_dev, float* eps_dev, int B, hipStream_t s,
                const StepOpts& o);
// One stage of a forward that dd_sample_early_exit_real drives block by block, on the B active slots of a chain whose step started with
// B_full images (the strides of the taps' tables): REAL_EMBED (x_img, y -> hand), REAL_TAPS (layer bi's head and probe into ee, finished at
// once), REAL_BLOCK (block bi: hand in, hand out), REAL_HEAD (the output head: eps).  The launches are those of run_backbone.
enum RealStageKind { REAL_EMBED, REAL_TAPS, REAL_BLOCK, REAL_HEAD };
struct RealStage {
    int kind, bi, B, B_full;
    const float* x_img = nullptr;
    const int64_t* y = nullptr;
    const EeTaps* ee = nullptr;
    float* eps = nullptr;
};
int real_exit_stage(dd_model* m, const Chain& ch, const RealStage& r, Handoff& hand, hipStream_t s);
int stage_inputs(dd_ctx* c, const float* x_dev, const int64_t* y_dev, int B, size_t x_elems, hipStream_t s, float** x_run,
                 const int64_t** y_run);
int stage_guided(dd_ctx* c, const float* x_dev, const int64_t* y_dev, int B, int B0, size_t chw, int null_label, hipStream_t s,
                 float** x_run, const int64_t** y_run);
int unstage_guided(dd_ctx* c, float* x_dev, const float* x_run, int B, int B0, size_t chw, hipStream_t s);
// The context's per-image seeds for a call of B images in this noise mode.  check: DD_ERR_INVALID where they are set, the call draws device
// noise and n != B -- before anything is enqueued.  stage: *seeds = the context's copy, refreshed from the caller's array on s (null where
// none are set or the call draws no device noise: DD_NOISE_BUFFER and DD_NOISE_NONE calls are what they are without them).
int check_image_seeds(dd_ctx* c, int noise_mode, int B);
int stage_image_seeds(dd_ctx* c, int noise_mode, hipStream_t s, const unsigned long long** seeds);

}  // namespace dd
#pragma GCC visibility pop
