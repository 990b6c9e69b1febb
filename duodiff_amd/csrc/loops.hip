// The device-resident sampling loops and scans: every dd_sample* entry point except dd_sample_step, dd_scan_error*, and dd_profile_steps*.
// Host code that enqueues launches; above forward.hip, below capi.hip (engine_state.h).  In this order:
//   - the half-batch chains: when a call splits (use_chains) and the one fork / join of the two streams (ChainFork);
//   - a loop as data (Loop): what each row runs (Program: the switch rule, a walk's jumps, block caching's reuse steps) and the callbacks
//     that differ between the entries; run_loop drives it -- staging, graph capture and replay, the timing events;
//   - the entries on run_loop: their checks (check_loop), the staging of tables and known regions, then dd_sample, the three dd_sample_affine
//     paths on one shared check and base loop, dd_sample_multistep, the two scans and dd_sample_early_exit;
//   - dd_sample_early_exit_real: an eager loop of its own on the same early-exit setup, scratch block and chain fork.
//
// Host-side restatement of: get_samples DDPM branch and backbone switch (reference sampler.py:128-139), the early-exit sampler (eesampler.py:56-81).
#include "../../include/duodiff.h"
#include "../../include/duodiff_dev.h"
#include "engine_state.h"
#include "ee_real.h"

#include <algorithm>
#include <array>
#include <chrono>
#include <functional>

using namespace dd;

namespace {

Mods guided(const dd_guidance* g) { return Mods{.g = g, .missing = g ? nullptr : "null dd_guidance"}; }
Mods autoguided(const dd_autoguidance* ag) { return Mods{.ag = ag, .missing = ag ? nullptr : "null dd_autoguidance"}; }
Mods in_region(const dd_guidance* g, const dd_autoguidance* ag, const dd_known_region* kr) { return Mods{.g = g, .ag = ag, .kr = kr, .region = true}; }
Mods thresholding(const dd_guidance* g, const dd_autoguidance* ag, const dd_known_region* kr, const dd_x0_threshold* thr) {
    return Mods{.g = g, .ag = ag, .kr = kr, .region = kr != nullptr, .thr = thr, .thresholded = true};
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
// The fork and the join of the two half-batch chains of a chained call (chained false: nothing).  fork() behind the staging copies and the
// state: the side stream starts behind them; join() in front of the tail: the caller's stream goes on behind the side stream.  A failure
// between the two must not leave the side stream running on the second chain's buffers behind the caller's back: the scope waits for it.
struct ChainFork {
    dd_ctx* c; hipStream_t s; bool chained; bool armed = false;
    int fork() {
        if (!chained) return DD_OK;
        DD_HIP(c, hipEventRecord(c->ev_fork, s));
        DD_HIP(c, hipStreamWaitEvent(c->side, c->ev_fork, 0));
        armed = true;
        return DD_OK;
    }
    int join() {
        if (!chained) return DD_OK;
        DD_HIP(c, hipEventRecord(c->ev_join, c->side));
        DD_HIP(c, hipStreamWaitEvent(s, c->ev_join, 0));
        armed = false;
        return DD_OK;
    }
    ~ChainFork() { if (armed && c->side) (void)hipStreamSynchronize(c->side); }
};

// the captured graph in `exec`, captured under the key `have`: reused if that is `key`, else captured now from enqueue()
template <typename F>
int capture_graph(dd_ctx* c, hipGraphExec_t& exec, GraphKey& have, const GraphKey& key, hipStream_t s, F&& enqueue) {
    if (exec && have == key) return DD_OK;
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
    have = key;
    ++c->graph_captures;
    return DD_OK;
}
// the model's captured step of this kind for this chain and key
template <typename F>
int get_graph(dd_ctx* c, dd_model* m, GraphKind kind, int chain, const GraphKey& key, hipStream_t s, F&& enqueue) {
    return capture_graph(c, m->graph[kind][chain], m->gkey[kind][chain], key, s, enqueue);
}

// One chain's share of a sampling loop's batch: the caller's images [b0, b0 + B), at x / y in the buffers the loop runs on
// (mods: the loop's, with the chain's share of the known region)
struct Slice { int chain, chains; float* x; const int64_t* y; int B, b0; Mods mods; };

// What a row of a sampling loop runs: a model's full step, a jump (dd_sample_affine_walk: no model), or a model's reuse step (block caching)
enum StepOp { STEP_FIRST = 0, STEP_LATE = 1, STEP_JUMP = 2, STEP_FIRST_REUSE = 3, STEP_LATE_REUSE = 4, STEP_OPS = 5 };
// a model's full step, its reuse step, and back
constexpr int reuse_of(int full) { return full == STEP_LATE ? STEP_LATE_REUSE : STEP_FIRST_REUSE; }
constexpr bool is_reuse(int op) { return op == STEP_FIRST_REUSE || op == STEP_LATE_REUSE; }
constexpr int full_of(int op) { return op == STEP_LATE_REUSE ? STEP_LATE : op == STEP_FIRST_REUSE ? STEP_FIRST : op; }

// The rows of a loop: a StepOp each.  switched: the program states the switch rule (switch_program) -- such a loop captures both models' full
// step whoever runs; late_behind: and that rule puts the switch behind the last step.
struct Program { std::vector<int> ops; bool switched = false, late_behind = false; };
// the switch rule: of `steps` rows the late model runs [switch_at, steps); switch_at == steps or -1: none
Program switch_program(int steps, int switch_at) {
    Program p{std::vector<int>((size_t)steps, STEP_FIRST), true, switch_at == steps};
    for (int k = switch_at; k >= 0 && k < steps; ++k) p.ops[k] = STEP_LATE;
    return p;
}
// the switch row of a table-driven loop's arguments, for switch_program (-1: the late model runs no row)
template <typename Args>
int switch_row(const Args* a) { return a->late && a->switch_after >= 0 && a->switch_after < a->n_steps ? a->switch_after : -1; }

// A sampling loop as run_loop drives it: the entry point has run its checks and supplies what differs between the loops
struct Loop {
    GraphKind kind;
    dd_model* first;
    dd_model* late;      // the model of the STEP_LATE rows, or null
    Program program;
    float* x_dev;
    const int64_t* y_dev;
    int B;
    Mods mods;           // (the early-exit loop: none)
    bool use_graph;
    std::function<hipError_t(StepState*, hipStream_t)> set_state;                   // a chain's step state at the start of the loop
    std::function<void(GraphKey&, const Slice&)> key;                                // the loop's own fields of a chain's graph key
    // one step of one chain.  reuse (block caching, a STEP_*_REUSE row): the model's reuse step -- with graphs its second captured graph
    // (GRAPH_AFFINE_REUSE)
    std::function<int(dd_model*, const Chain&, const Slice&, bool reuse, hipStream_t)> step;
    std::function<int(int chains, hipStream_t)> tail = nullptr;                      // behind the join of the chains
    // one jump of one chain (a STEP_JUMP row).  With graphs the row replays the context's captured jump of the chain (dd_ctx::jump_graph, keyed
    // like a step's graph)
    std::function<int(const Chain&, const Slice&, hipStream_t)> jump = nullptr;
    // called once the chains are decided and before the loop captures, stages or launches anything, with their number and chain 0's images:
    // refuses the call or admits it
    std::function<int(int chains, int B0, hipStream_t)> admit = nullptr;
};

// The graphs a call captures, by op.  A loop given by the switch rule captures both models' full step (the late model's where it has one) even
// when no row runs it; a walk or cached loop captures what its rows name.  late == first is one model: either name stands for both.
std::array<bool, STEP_OPS> captured_ops(const Loop& L) {
    std::array<bool, STEP_OPS> uses{};
    uses[STEP_FIRST] = uses[STEP_LATE] = L.program.switched;
    for (int op : L.program.ops) uses[op] = true;
    if (L.late == L.first) {
        uses[STEP_FIRST] = uses[STEP_LATE] = uses[STEP_FIRST] || uses[STEP_LATE];
        uses[STEP_FIRST_REUSE] = uses[STEP_LATE_REUSE] = uses[STEP_FIRST_REUSE] || uses[STEP_LATE_REUSE];
    }
    return uses;
}

// Every dd_sample* loop that replays captured steps and both scans: staging, the half-batch chains, graph capture, the rows of the program
// (replayed or eager), timing.  ev[0] .. ev[2] bracket the loop; ev[1] splits it into the first and the late model's share.
int run_loop(dd_ctx* c, const Loop& L, hipStream_t s) {
    const dd_guidance* g = L.mods.g;
    const dd_autoguidance* ag = L.mods.ag;
    const std::vector<int>& ops = L.program.ops;
    const int steps = (int)ops.size();
    // Two half-batch chains (graph replays only).  Images are independent and a row's path through the kernels does not depend on the
    // batch size, so chain 0 = images [0, B0) on the caller's stream and chain 1 = images [B0, B) on the context's side stream compute
    // bit for bit what the undivided batch computes (Philox pixel ids carry the image offset) -- with the two chains free to drift apart,
    // so that one's HBM-bound phases (row prologues / epilogues, attention row fetch) run under the other's MFMA phases.
    // Guided: the decisions are made on the 2 B backbone rows and the split is by image (chain 0 takes the larger half, on the workspace
    // sized for max_batch >= 2 B rows; the second chain's workspace holds (max_batch + 1) / 2 rows >= 2 * floor(B / 2)).
    const bool ee = L.kind == GRAPH_EARLY_EXIT || L.kind == GRAPH_SCAN_EXITS;      // the loops of an early-exit model
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
    if (L.admit && (rc = L.admit(chains, B0, s))) return rc;
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
        const auto uses = captured_ops(L);
        for (int k = 0; k < chains; ++k) {
            const Slice sl = slice(k);
            GraphKey key{sl.x, sl.y, sl.B, 0, 0, cus, nullptr};
            key.b0 = sl.b0;
            key.guide(g);
            key.perturb(pag);
            key.kx0 = sl.mods.kn.x0; key.kmask = sl.mods.kn.mask; key.ktab = sl.mods.kn.ktab;
            key.seeds = L.mods.seeds;
            L.key(key, sl);
            if (uses[STEP_JUMP]) {
                GraphKey jkey = key;
                jkey.jchans = L.first->cfg.in_chans; jkey.jsize = L.first->cfg.img_size;
                if ((rc = capture_graph(c, c->jump_graph[k], c->jump_key[k], jkey, s, [&] { return L.jump(chain(L.first, k), sl, s); }))) return rc;
            }
            for (dd_model* m : {L.first, L.late}) {
                const int full = m == L.first ? STEP_FIRST : STEP_LATE;
                if (!m || !(uses[full] || uses[reuse_of(full)])) continue;
                if (k && (rc = ensure_chain_ws(c, m, s))) return rc;
                GraphKey mkey = key;
                if (ag) {   // the step of the guide model itself is the unguided loop's step, under the unguided loop's key
                    if (m->cfg.num_classes <= 0) mkey.y = nullptr;
                    if (m != ag->guide) {
                        if (k && (rc = ensure_chain_ws(c, ag->guide, s))) return rc;
                        mkey.aguide = ag->guide; mkey.aserial = ag->guide->serial; mkey.gscale = __builtin_bit_cast(unsigned, ag->scale);
                    }
                }
                if (uses[full] && (rc = get_graph(c, m, L.kind, k, mkey, s, [&] { return L.step(m, chain(m, k), sl, false, s); }))) return rc;
                if (uses[reuse_of(full)] && (rc = get_graph(c, m, GRAPH_AFFINE_REUSE, k, mkey, s, [&] { return L.step(m, chain(m, k), sl, true, s); }))) return rc;
            }
        }
    }
    for (int k = 0; k < chains; ++k) DD_HIP(c, L.set_state(c->st[k], s));
    ChainFork chain_fork{c, s, chained};
    if ((rc = chain_fork.fork())) return rc;
    DD_HIP(c, hipEventRecord(c->ev[0], s));
    // ev[1] is recorded in front of row `split`, the first row the late model runs.  It runs none: behind the last row and in front of the
    // join (split == steps) where the switch rule puts the switch there, else behind the join and the tail (split < 0).
    int split = L.program.late_behind ? steps : -1;
    for (int k = steps; k-- > 0;)
        if (full_of(ops[k]) == STEP_LATE) split = k;
    for (int k = 0; k < steps; ++k) {
        if (k == split) DD_HIP(c, hipEventRecord(c->ev[1], s));
        const bool jump = ops[k] == STEP_JUMP, reuse = is_reuse(ops[k]);
        dd_model* cur = full_of(ops[k]) == STEP_LATE ? L.late : L.first;       // (a jump: no model runs)
        if (L.use_graph) {
            const hipGraphExec_t* graphs = jump ? c->jump_graph : cur->graph[reuse ? GRAPH_AFFINE_REUSE : L.kind];
            DD_HIP(c, hipGraphLaunch(graphs[0], s));
            if (chained) DD_HIP(c, hipGraphLaunch(graphs[1], c->side));
        } else if ((rc = jump ? L.jump(chain(cur, 0), slice(0), s) : L.step(cur, chain(cur, 0), slice(0), reuse, s))) {
            return rc;
        }
    }
    if (split == steps) DD_HIP(c, hipEventRecord(c->ev[1], s));
    if ((rc = chain_fork.join())) return rc;
    if (L.tail && (rc = L.tail(chains, s))) return rc;
    if (split < 0) DD_HIP(c, hipEventRecord(c->ev[1], s));
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
// Where a chain's forward writes eps and the taps it takes (taps.cls null: none, a plain model's forward) -- ee_block: the block of the chain
// that runs images [b0, b0 + B) in the model's early-exit scratch, eps | cls | outs
struct EeBlock { float* eps; EeTaps taps; };
EeBlock ee_block(const dd_model* m, int b0, int B) {
    const size_t chw = (size_t)m->cfg.in_chans * m->cfg.img_size * m->cfg.img_size;
    float* eps = m->ee_ws + ee_scratch_elems(m, b0);
    float* cls = eps + (size_t)B * chw;                 // [depth, B]
    return EeBlock{eps, EeTaps{cls, cls + (size_t)m->cfg.depth * B, 0}};
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
    ChainFork chain_fork{c, s, chained};
    if ((rc = chain_fork.fork())) return rc;
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
    if (rc || (rc = chain_fork.join())) return rc;
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
    if ((rc = check_image_seeds(c, a->noise_mode, a->B))) return rc;
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
// (bc, dd_sample_affine_cached: the row's cache op and the bits of its extrapolation weight in the two spare words)
template <typename Args>
int upload_atab(dd_ctx* c, const Args* a, hipStream_t s, const dd_block_cache* bc = nullptr) {
    return upload_rows(c, c->atab, (size_t)a->n_steps + 1, s, [a, bc](size_t k) {
        return k < (size_t)a->n_steps ? AffineRow{a->t[k], a->a[k], a->b[k], a->c[k], a->noise[k] ? 1 : 0, a->counter_base + (int)k,
                                                  bc ? bc->op[k] : 0, bc ? __builtin_bit_cast(int, bc->w[k]) : 0}
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
    if ((rc = stage_image_seeds(c, a->noise_mode, (hipStream_t)stream, &mo.seeds))) return rc;
    if ((rc = stage_known(c, mo, a->first, a->B, 1000, (hipStream_t)stream, known_row))) return rc;
    Loop L{GRAPH_DDPM, a->first, switching ? a->late : nullptr, switch_program(n, switch_here ? a->t_start - t_sw + 1 : -1), a->x_dev, a->y_dev,
           a->B, mo, a->use_graph != 0};
    L.set_state = [&](StepState* st, hipStream_t s) { return launch_set_state(st, a->t_start, (unsigned long long)a->seed, s); };
    L.key = [&](GraphKey& k, const Slice&) { k.noise = a->noise_mode; k.variance = a->variance; };
    L.step = [&](dd_model* m, const Chain& ch, const Slice& sl, bool, hipStream_t s) {
        return enqueue_step(c, m, ch, sl.x, sl.y, sl.B, s,
                            {.mods = sl.mods, .noise_mode = a->noise_mode, .variance = a->variance, .advance = 1, .b0 = sl.b0});
    };
    return run_loop(c, L, (hipStream_t)stream);
}

// What dd_sample_affine, dd_sample_affine_walk and dd_sample_affine_cached share.  The loop's checks, with the entry's two rejection texts,
int check_affine(dd_ctx* c, const dd_affine_sample_args* a, const Mods& mo, const char* no_early_exit, const char* host_noise) {
    return check_loop(c, a, mo, no_early_exit, host_noise, [&] { return check_table(c, a); });
}
// and behind them: the seeds, the step table (bc: upload_atab) and the known rows staged on s, and the loop of switch_after's rule over that
// table (two half-batch chains, as dd_sample: both read the one step table; each has its own step index and Philox image offset)
int affine_loop(dd_ctx* c, const dd_affine_sample_args* a, Mods mo, hipStream_t s, const dd_block_cache* bc, Loop& L) {
    int rc = stage_image_seeds(c, a->noise_mode, s, &mo.seeds);
    if (rc || (rc = upload_atab(c, a, s, bc)) || (rc = stage_table_known(c, mo, a->first, a->B, a->n_steps, s))) return rc;
    const AffineRow* atab = c->atab.dev.p;
    const int sw = switch_row(a);
    L = Loop{GRAPH_AFFINE, a->first, sw >= 0 ? a->late : nullptr, switch_program(a->n_steps, sw), a->x_dev, a->y_dev, a->B, mo, a->use_graph != 0};
    L.set_state = [=](StepState* st, hipStream_t ss) { return launch_set_state_table(st, atab, (unsigned long long)a->seed, ss); };
    L.key = [=](GraphKey& k, const Slice&) { k.noise = a->noise_mode; k.atab = atab; };
    L.step = [=](dd_model* m, const Chain& ch, const Slice& sl, bool, hipStream_t ss) {
        return enqueue_step(c, m, ch, sl.x, sl.y, sl.B, ss, {.mods = sl.mods, .noise_mode = a->noise_mode, .advance = 1, .atab = atab, .b0 = sl.b0});
    };
    return DD_OK;
}

// dd_sample_affine and its _guided, _autoguided, _region and _perturbed forms: one path
int sample_affine(dd_ctx* c, const dd_affine_sample_args* a, Mods mo, void* stream) {
    int rc = check_affine(c, a, mo, nullptr, "dd_sample_affine generates noise on the device; for host noise drive dd_forward + dd_affine_step");
    Loop L;
    if (rc || (rc = affine_loop(c, a, mo, (hipStream_t)stream, nullptr, L))) return rc;
    return run_loop(c, L, (hipStream_t)stream);
}

// dd_sample_affine_walk: its own checks, in front of the loop's (the table's pointers and n_steps are checked there: unreadable ones are left
// to it), then dd_sample_affine's loop with the rows the walk names: a jump row runs launch_jump, a step row the model w->late names (null:
// switch_after's rule)
int sample_affine_walk(dd_ctx* c, const dd_affine_sample_args* a, const dd_guidance* g, const dd_autoguidance* ag, const dd_known_region* kr,
                       const dd_walk* w, void* stream) {
    if (!c) return DD_ERR_INVALID;
    if (!w || !w->jump) return ctx_fail(c, DD_ERR_INVALID, "null dd_walk / null jump array");
    if (!a) return DD_ERR_INVALID;
    if (a->b && a->n_steps >= 1 && a->n_steps <= (1 << 20)) {
        for (int k = 0; k < a->n_steps; ++k) {
            if (w->jump[k]) {
                if (a->b[k] != 0.f) return ctx_fail(c, DD_ERR_INVALID, "row " + std::to_string(k) + " is a jump with b != 0: a jump runs no model");
            } else if (w->late) {
                if (w->late[k] != 0 && w->late[k] != 1) return ctx_fail(c, DD_ERR_INVALID, "late[" + std::to_string(k) + "] is outside {0, 1}");
                if (w->late[k] == 1 && !a->late) return ctx_fail(c, DD_ERR_INVALID, "late[" + std::to_string(k) + "] is 1 without a late model");
            }
        }
    }
    if (g && ag) return ctx_fail(c, DD_ERR_INVALID, "classifier-free guidance and autoguidance are exclusive");
    const Mods mo{.g = g, .ag = ag, .kr = kr, .region = kr != nullptr};
    int rc = check_affine(c, a, mo, "resampling jumps are not supported for early-exit models",
                          "dd_sample_affine_walk generates noise on the device; for host noise drive dd_forward, dd_affine_step, dd_known_blend and dd_jump_step");
    if (rc) return rc;
    if (a->first->cfg.in_chans > 4) return ctx_fail(c, DD_ERR_UNSUPPORTED, "a resampling jump draws one Philox block per pixel: at most 4 channels");
    hipStream_t s = (hipStream_t)stream;
    Loop L;
    if ((rc = affine_loop(c, a, mo, s, nullptr, L))) return rc;
    for (int k = 0; k < a->n_steps; ++k) {
        if (w->jump[k]) L.program.ops[k] = STEP_JUMP;
        else if (w->late) L.program.ops[k] = w->late[k] ? STEP_LATE : STEP_FIRST;
    }
    L.program.switched = false;          // (the call captures what its rows name)
    if (w->late) L.late = a->late;       // (the rows name their model; null where no row runs it: checked)
    const AffineRow* atab = c->atab.dev.p;
    L.jump = [=](const Chain& ch, const Slice& sl, hipStream_t ss) -> int {      // (guided: the chain's twins stand sl.B images on)
        DD_HIP(c, launch_jump(sl.x, ch.st, atab, sl.mods.seeds, sl.B, a->first->cfg.in_chans, a->first->cfg.img_size, sl.b0, g ? sl.B : 0,
                              a->noise_mode, ss));
        return DD_OK;
    };
    return run_loop(c, L, s);
}

// Block caching: each cache a call runs on, and what the call's rows leave in it
using CacheWalk = std::vector<std::pair<BlockCache*, BlockCache>>;
// The rows of a cached loop walked over its models' cache validity, for the chains run_loop has decided on (Loop::admit): a reuse row needs a
// refresh of its model, chain geometry and K in front of it -- in this call or left by an earlier one -- and an extrapolating row two of them
int walk_cache_validity(dd_ctx* c, const Loop& L, const dd_block_cache* bc, int chains, int B0, hipStream_t s, CacheWalk& walked) {
    dd_model* models[2] = {L.first, L.late};
    BlockCache sim[2][2];
    for (int ck = 0; ck < chains; ++ck) {
        const int b0 = ck ? B0 : 0, Bk = ck ? L.B - B0 : B0, rows = L.mods.g ? 2 * Bk : Bk;
        for (int i = 0; i < 2; ++i) if (models[i]) sim[ck][i] = models[i]->cache[ck];
        for (int k = 0; k < (int)L.program.ops.size(); ++k) {
            const int i = (full_of(L.program.ops[k]) == STEP_LATE && models[1] != models[0]) ? 1 : 0;
            BlockCache& v = sim[ck][i];
            if (bc->op[k] == CACHE_REFRESH) { v.refresh(bc->blocks, rows, b0, Bk, bc->order == 1); continue; }
            if (!v.holds(bc->blocks, rows, b0, Bk))
                return ctx_fail(c, DD_ERR_INVALID, "block caching: row " + std::to_string(k) + " is a reuse step, and its model holds no refresh of this batch and these blocks");
            if (bc->op[k] == CACHE_EXTRAPOLATE && !v.has_prev)
                return ctx_fail(c, DD_ERR_INVALID, "block caching: row " + std::to_string(k) + " extrapolates, and its model holds no second refresh of this batch and these blocks");
        }
    }
    for (int ck = 0; ck < chains; ++ck)
        for (int i = 0; i < 2; ++i) {
            if (!models[i] || (i && models[1] == models[0])) continue;
            if (int r = ensure_block_cache(c, models[i], ck, s)) { walked.clear(); return r; }
            walked.push_back({&models[i]->cache[ck], sim[ck][i]});
        }
    return DD_OK;
}
// The walk becomes the models' validity once the whole loop is enqueued (rc: run_loop's).  A call that fails behind the walk (a capture, a
// copy, a launch) may have rotated or half-written the buffers, so they then hold nothing.
void commit_cache_walk(const CacheWalk& walked, int rc) {
    for (auto& [d, v] : walked) {
        if (rc) { d->has_last = d->has_prev = false; continue; }
        d->K = v.K; d->rows = v.rows; d->b0 = v.b0; d->B = v.B; d->has_last = v.has_last; d->has_prev = v.has_prev;
    }
}

// dd_sample_affine_cached: its own checks, in front of the loop's (the table's pointers and n_steps are checked there), then dd_sample_affine's
// loop with the cache: a row with op != 0 runs its model's reuse step.  What needs the models or the chains is checked behind the loop's
// checks: K against every model that runs a step before anything is enqueued, the walk over the cache validity (Loop::admit) behind the copies
// of the table, the seeds and the known rows into the context's staging buffers and in front of every capture, copy or launch that touches x, a
// workspace or a cache.
int sample_affine_cached(dd_ctx* c, const dd_affine_sample_args* a, const dd_guidance* g, const dd_known_region* kr, const dd_block_cache* bc,
                         void* stream) {
    if (!c) return DD_ERR_INVALID;
    if (!bc || !bc->op || !bc->w) return ctx_fail(c, DD_ERR_INVALID, "null dd_block_cache / null op or w array");
    if (!a) return DD_ERR_INVALID;
    if (bc->order != 0 && bc->order != 1) return ctx_fail(c, DD_ERR_INVALID, "block caching: order outside {0, 1}");
    if (a->n_steps >= 1 && a->n_steps <= (1 << 20)) {
        for (int k = 0; k < a->n_steps; ++k) {
            if (bc->op[k] < CACHE_REFRESH || bc->op[k] > CACHE_EXTRAPOLATE)
                return ctx_fail(c, DD_ERR_INVALID, "block caching: op[" + std::to_string(k) + "] is outside {0, 1, 2}");
            if (bc->op[k] == CACHE_EXTRAPOLATE && bc->order == 0)
                return ctx_fail(c, DD_ERR_INVALID, "block caching: op[" + std::to_string(k) + "] extrapolates under order 0");
        }
    }
    const Mods mo{.g = g, .kr = kr, .region = kr != nullptr};
    int rc = check_affine(c, a, mo, "block caching is not supported for early-exit models",
                          "dd_sample_affine_cached generates noise on the device; for host noise drive dd_forward_cached + dd_affine_step");
    if (rc) return rc;
    const int sw = switch_row(a);
    for (int k = 0; k < a->n_steps; ++k)
        if ((rc = check_cached(c, sw >= 0 && k >= sw ? a->late : a->first, bc->blocks))) return rc;
    hipStream_t s = (hipStream_t)stream;
    Loop L;
    if ((rc = affine_loop(c, a, mo, s, bc, L))) return rc;
    for (int k = 0; k < a->n_steps; ++k)
        if (bc->op[k]) L.program.ops[k] = reuse_of(L.program.ops[k]);
    L.program.switched = false;          // (the call captures what its rows name)
    const AffineRow* atab = c->atab.dev.p;
    L.key = [=](GraphKey& k, const Slice&) { k.noise = a->noise_mode; k.atab = atab; k.cblocks = bc->blocks; k.corder = bc->order; };
    L.step = [=](dd_model* m, const Chain& ch, const Slice& sl, bool reuse, hipStream_t ss) {
        // order 1: a refresh rotates prev <- last first, and a reuse goes through the kernel, which reads the row's op and w
        const bool order1 = bc->order == 1;
        const CacheUse cu{bc->blocks, reuse, !reuse && order1, reuse && order1, 0.f, reuse && order1 ? atab : nullptr};
        return enqueue_step(c, m, ch, sl.x, sl.y, sl.B, ss, {.mods = sl.mods, .cache = cu, .noise_mode = a->noise_mode, .advance = 1, .atab = atab, .b0 = sl.b0});
    };
    CacheWalk walked;
    L.admit = [&](int chains, int B0, hipStream_t ss) { return walk_cache_validity(c, L, bc, chains, B0, ss, walked); };
    rc = run_loop(c, L, s);
    commit_cache_walk(walked, rc);
    return rc;
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
    const int sw = switch_row(a);
    if ((rc = stage_image_seeds(c, a->noise_mode, s, &mo.seeds))) return rc;
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
    Loop L{GRAPH_MULTISTEP, a->first, sw >= 0 ? a->late : nullptr, switch_program(n, sw), a->x_dev, a->y_dev, a->B, mo, a->use_graph != 0};
    L.set_state = [&](StepState* st, hipStream_t ss) { return launch_set_state_table(st, atab, (unsigned long long)a->seed, ss); };
    L.key = [&](GraphKey& k, const Slice&) {
        k.noise = a->noise_mode; k.atab = atab; k.aux0 = htab; k.aux1 = h_run;
        if (mo.thresholded) {
            k.tmode = mo.thr->mode; k.tscratch = m_run;
            k.tq = __builtin_bit_cast(unsigned, mo.thr->quantile); k.tr = __builtin_bit_cast(unsigned, mo.thr->range);
            k.ts = __builtin_bit_cast(unsigned, mo.thr->s_max);
        }
    };
    L.step = [&](dd_model* m, const Chain& ch, const Slice& sl, bool, hipStream_t ss) {
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

// The denoising-error scans (dd_scan_error, dd_scan_error_early_exit) as one more loop of run_loop.  A step is diffuse -> forward_eps ->
// the entry's error kernel (scan.hip); the images x0 are staged like a known image (k_stage: a later call with other tensors of the same
// shape replays the same graphs), the rows live in the context's stab, and x_t with the entry's results behind it in its scan_ws
// (engine_state.h has the layouts).  With graphs run_loop's staged x is the chain's x_t buffer (scan_ws' x_t part then only passes through
// its copies); eagerly the loop runs on scan_ws itself.  The result rows are disjoint per image: two half-batch chains need no join kernel.
//
// The checks of a scan behind check_call, in this order (Args: dd_scan_args or dd_scan_exits_args, one layout up to `reserved`): the
// pointers (results: the entry's own result tensors are all there), the step count, the counter base, the noise mode, the entry's own
// checks, the image seeds and the shape the scan kernels take
template <typename Args, typename Own>
int check_scan(dd_ctx* c, const Args* a, const char* entry, bool results, Own&& own_checks) {
    if (!results || !a->x0_dev || !a->t || !a->ka || !a->kb || !a->tz || !a->t0 || !a->tx) return ctx_fail(c, DD_ERR_INVALID, "null tensor / table");
    if (a->n_steps < 1 || a->n_steps > (1 << 20)) return ctx_fail(c, DD_ERR_INVALID, "n_steps outside [1, 2^20]");
    if (a->counter_base < 0 || a->counter_base > (1 << 20)) return ctx_fail(c, DD_ERR_INVALID, "counter_base outside [0, 2^20]");
    if (a->noise_mode != DD_NOISE_PHILOX)
        return ctx_fail(c, DD_ERR_INVALID, std::string(entry) + " draws its noise on the device: noise_mode must be DD_NOISE_PHILOX");
    int rc = own_checks();
    if (rc || (rc = check_image_seeds(c, a->noise_mode, a->B))) return rc;
    const dd_config& cfg = a->model->cfg;
    if (cfg.in_chans < 1 || cfg.in_chans > 4 || (size_t)cfg.in_chans * cfg.img_size * cfg.img_size > ((size_t)1 << 24))
        return ctx_fail(c, DD_ERR_UNSUPPORTED, "the scan kernels take 1..4 channels and at most 2^24 elements per image");
    return DD_OK;
}

// What a checked scan runs on: the staged seeds, row table and images (chw elements each, elems in all), and scan_ws as x_t | `results`
struct ScanStage { const unsigned long long* seeds = nullptr; const ScanRow* tab; const float* x0; float* results; size_t chw, elems; };
// ... staged on s: the image seeds, `rows` rows (row(i) each) in stab, x0 in k_stage, and scan_ws grown to x_t and result_elems behind it
template <typename Args, typename F>
int stage_scan(dd_ctx* c, const Args* a, size_t rows, F&& row, size_t result_elems, hipStream_t s, ScanStage* g) {
    const dd_config& cfg = a->model->cfg;
    g->chw = (size_t)cfg.in_chans * cfg.img_size * cfg.img_size;
    g->elems = (size_t)a->B * g->chw;
    int rc = stage_image_seeds(c, a->noise_mode, s, &g->seeds);
    if (rc || (rc = upload_rows(c, c->stab, rows, s, row))) return rc;
    if ((rc = c->k_stage.grow(c, g->elems))) return rc;
    DD_HIP(c, hipMemcpyAsync(c->k_stage.p, a->x0_dev, g->elems * sizeof(float), hipMemcpyDeviceToDevice, s));
    if ((rc = c->scan_ws.grow(c, g->elems + result_elems))) return rc;
    g->tab = c->stab.dev.p; g->x0 = c->k_stage.p; g->results = c->scan_ws.p + g->elems;
    return DD_OK;
}

// a result table of a scan, copied to the caller's tensor behind the loop, so that a captured step never names it
struct ScanOut { float* dst; const float* src; size_t elems; };

// The loop of a staged scan: `kind`'s graphs, the step state started at row first_row, key(k) the entry's own key fields, forward(m, slice)
// the chain's EeBlock (no taps: a plain model's), error(f, x0, chain, slice, s) the launch that ends the step, and outs
template <typename Args, typename Key, typename Forward, typename Error>
int run_scan(dd_ctx* c, const Args* a, const ScanStage& g, GraphKind kind, int first_row, Key&& key, Forward&& forward, Error&& error,
             std::initializer_list<ScanOut> outs, hipStream_t s) {
    const int C = a->model->cfg.in_chans, S = a->model->cfg.img_size;
    Loop L{kind, a->model, nullptr, switch_program(a->n_steps, -1), c->scan_ws.p, a->y_dev, a->B, Mods{.seeds = g.seeds}, a->use_graph != 0};
    L.set_state = [&](StepState* st, hipStream_t ss) { return launch_set_state_scan(st, g.tab, (unsigned long long)a->seed, ss, first_row); };
    L.key = [&](GraphKey& k, const Slice& sl) {
        k.noise = a->noise_mode; k.atab = g.tab; k.kx0 = g.x0 + (size_t)sl.b0 * g.chw;
        key(k);
        if (sl.chains == 2 && sl.chain == 0) k.b0 = -1;     // (chain 0 of two writes rows of 2 B images -- not the whole batch's graph)
    };
    L.step = [&](dd_model* mm, const Chain& ch, const Slice& sl, bool, hipStream_t ss) -> int {
        const float* x0 = g.x0 + (size_t)sl.b0 * g.chw;
        const EeBlock f = forward(mm, sl);
        DD_HIP(c, launch_scan_diffuse(x0, sl.x, ch.st, g.tab, sl.mods.seeds, sl.B, C, S, sl.b0, ss));
        if (int r = forward_eps(c, mm, ch, sl.x, sl.y, f.eps, sl.B, ss, {.ee = f.taps.cls ? &f.taps : nullptr})) return r;
        DD_HIP(c, error(f, x0, ch, sl, ss));
        return DD_OK;
    };
    L.tail = [&](int, hipStream_t ss) -> int {
        for (const ScanOut& o : outs) DD_HIP(c, hipMemcpyAsync(o.dst, o.src, o.elems * sizeof(float), hipMemcpyDeviceToDevice, ss));
        return DD_OK;
    };
    return run_loop(c, L, s);
}

// dd_scan_error: a plain model; the step's index is the row, and scan_ws holds x_t | eps | err [n, B]
int scan_error(dd_ctx* c, const dd_scan_args* a, void* stream) {
    if (!c || !a) return DD_ERR_INVALID;
    dd_model* m = a->model;
    if (m && m->ctx == c && m->ee_type >= 0)
        return ctx_fail(c, DD_ERR_INVALID, "dd_scan_error takes a plain model, not one created with dd_model_enable_early_exit");
    int rc = check_call(c, m, a->B, a->y_dev);
    if (rc || (rc = check_scan(c, a, "dd_scan_error", a->err_dev != nullptr, [] { return DD_OK; }))) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int n = a->n_steps, C = m->cfg.in_chans, S = m->cfg.img_size;
    const size_t err_elems = (size_t)n * a->B;
    ScanStage g;
    // n rows + one more whose timestep the last step hands on (never used), as the step table of dd_sample_affine
    rc = stage_scan(c, a, (size_t)n + 1, [a, n](size_t k) {
        return k < (size_t)n ? ScanRow{a->t[k], a->ka[k], a->kb[k], a->tz[k], a->t0[k], a->tx[k], a->counter_base + (int)k, 0}
                             : ScanRow{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0, 0};
    }, (size_t)a->B * C * S * S + err_elems, s, &g);
    if (rc) return rc;
    float* eps_run = g.results;
    float* err_run = eps_run + g.elems;
    return run_scan(c, a, g, GRAPH_SCAN, 0, [&](GraphKey& k) { k.aux0 = err_run; k.aux1 = eps_run; },
                    [&](dd_model*, const Slice& sl) { return EeBlock{eps_run + (size_t)sl.b0 * g.chw, {}}; },
                    [&](const EeBlock& f, const float* x0, const Chain& ch, const Slice& sl, hipStream_t ss) {
                        return launch_scan_error(x0, f.eps, err_run, ch.st, g.tab, sl.mods.seeds, sl.B, C, S, sl.b0, a->B, 1, ss);
                    },
                    {{a->err_dev, err_run, err_elems}}, s);
}
// the early-exit scratch of a model (eps | cls | outs per chain, then dd_sample_early_exit's two sum tables), allocated on first use
int ensure_ee_ws(dd_ctx* c, dd_model* m) {
    const size_t tab = (size_t)1000 * m->cfg.depth;
    if (!m->ee_ws) DD_HIP(c, hipMalloc((void**)&m->ee_ws, (ee_scratch_elems(m, m->cfg.max_batch) + 2 * tab) * sizeof(float)));
    return DD_OK;
}

// dd_scan_error_early_exit: an early-exit model.  The step state holds the integer TIMESTEP, not the step's index (the per-timestep probe
// tables of the forward read it), so the row table is indexed by timestep -- 1000 rows of which the grid's are filled, each naming the
// next, and the base row with the call's counter_base.  The taps go to the model's early-exit scratch (each chain's block, as
// dd_sample_early_exit), and scan_ws holds x_t | mse | target | pred.
int scan_exits(dd_ctx* c, const dd_scan_exits_args* a, void* stream) {
    if (!c || !a) return DD_ERR_INVALID;
    dd_model* m = a->model;
    int rc = check_call(c, m, a->B, a->y_dev);
    if (rc) return rc;
    if (m->ee_type < 0) return ctx_fail(c, DD_ERR_STATE, "model was not created with dd_model_enable_early_exit");
    std::vector<int> at(SCAN_EXITS_ROWS, -1);       // timestep -> its step in the call
    rc = check_scan(c, a, "dd_scan_error_early_exit", a->mse_dev && a->target_dev && a->pred_dev, [&]() -> int {
        for (int k = 0; k < a->n_steps; ++k) {
            const float t = a->t[k];
            if (!(t >= 0.f && t <= 999.f) || t != (float)(int)t)
                return ctx_fail(c, DD_ERR_INVALID, "timestep " + std::to_string(k) + " is not an integer in [0, 999]: the probe tables are indexed by it");
            if (at[(int)t] >= 0) return ctx_fail(c, DD_ERR_INVALID, "timestep " + std::to_string((int)t) + " occurs twice");
            at[(int)t] = k;
        }
        return DD_OK;
    });
    if (rc) return rc;
    const int n = a->n_steps, C = m->cfg.in_chans, S = m->cfg.img_size, depth = m->cfg.depth, E = depth + 1;
    if (E > 32) return ctx_fail(c, DD_ERR_UNSUPPORTED, "the early-exit scan takes at most 32 exits (depth + 1)");
    hipStream_t s = (hipStream_t)stream;
    if ((rc = ensure_ee_ws(c, m))) return rc;
    const size_t mse_elems = (size_t)n * E * a->B, pred_elems = (size_t)n * depth * a->B;
    ScanStage g;
    rc = stage_scan(c, a, (size_t)SCAN_EXITS_ROWS + 1, [&](size_t t) {
        if (t == (size_t)SCAN_EXITS_ROWS) return ScanRow{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, a->counter_base, 0};
        const int k = at[t];
        if (k < 0) return ScanRow{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0, 0};
        // (the last step hands on the first timestep: a valid row, never used)
        return ScanRow{a->t[k], a->ka[k], a->kb[k], a->tz[k], a->t0[k], a->tx[k], a->counter_base + k, (int)a->t[k + 1 < n ? k + 1 : 0]};
    }, 2 * mse_elems + pred_elems, s, &g);
    if (rc) return rc;
    float* mse_run = g.results;
    float* tgt_run = mse_run + mse_elems;
    float* pred_run = tgt_run + mse_elems;
    return run_scan(c, a, g, GRAPH_SCAN_EXITS, (int)a->t[0], [&](GraphKey& k) { k.variance = n; k.aux0 = mse_run; k.aux1 = m->ee_ws; },
                    [&](dd_model* mm, const Slice& sl) { return ee_block(mm, sl.b0, sl.B); },
                    [&](const EeBlock& f, const float* x0, const Chain& ch, const Slice& sl, hipStream_t ss) {
                        return launch_scan_exits_error(x0, f.taps.outs, f.eps, f.taps.cls, mse_run, tgt_run, pred_run, ch.st, g.tab, sl.mods.seeds, sl.B, C, S,
                                                       E, sl.b0, a->B, 1, ss);
                    },
                    {{a->mse_dev, mse_run, mse_elems}, {a->target_dev, tgt_run, mse_elems}, {a->pred_dev, pred_run, pred_elems}}, s);
}

// One early-exit sampling step on the device (reference eesampler.py:56-81): EarlyExitUViT.forward with every head and
// probe -> per-sample exit selection -> DDPM update with the selected output; rows t of the two log tables are written.
// b0 / B_all: the chain's first image within the whole batch (its scratch block: ee_block) and the whole batch (idx_tab rows are B_all wide);
// seeds: the whole batch's staged per-image seeds or null; sums: err_tab is the chain's table of per-layer SUMS (launch_ee_mean_combine joins the chains)
int enqueue_ee_step(dd_ctx* c, dd_model* m, const Chain& ch, float* x, const int64_t* y, float thr, float* err_tab, int32_t* idx_tab,
                    int noise_mode, int B, hipStream_t s, int b0, int B_all, bool sums, const unsigned long long* seeds) {
    const EeBlock blk = ee_block(m, b0, B);
    if (int rc = forward_eps(c, m, ch, x, y, blk.eps, B, s, {.ee = &blk.taps})) return rc;
    // exit layer per image, the selected output and the DDPM update in one launch (dd_early_exit_select + the step kernel, fused: same arithmetic)
    DD_HIP(c, launch_ee_select_step(x, blk.taps.outs, blk.eps, blk.taps.cls, thr, m->cfg.depth, idx_tab, err_tab, B_all, b0, sums, ch.st, c->coef, B,
                                    m->cfg.in_chans, m->cfg.img_size, noise_mode, 1, s, seeds));
    return DD_OK;
}

// What dd_sample_early_exit and dd_sample_early_exit_real (`entry`: the one that is called) share in front of their loops: the checks, in this
// order and with the entry's own between them -- behind_tensor() behind the check of x_dev, behind_noise() behind the noise mode's -- then the
// image seeds staged on s and the model's early-exit scratch
int ee_sample_setup(dd_ctx* c, const dd_ee_sample_args* a, const char* entry, hipStream_t s, const unsigned long long** seeds,
                    const std::function<int()>& behind_tensor = nullptr, const std::function<int()>& behind_noise = nullptr) {
    if (!c || !a) return DD_ERR_INVALID;
    dd_model* m = a->model;
    int rc = check_call(c, m, a->B, a->y_dev);
    if (rc) return rc;
    if (m->ee_type < 0) return ctx_fail(c, DD_ERR_STATE, "model was not created with dd_model_enable_early_exit");
    if (!a->x_dev) return ctx_fail(c, DD_ERR_INVALID, "null tensor");
    if (behind_tensor && (rc = behind_tensor())) return rc;
    if (a->t_start > 999 || a->t_end < 0 || a->t_end > a->t_start) return ctx_fail(c, DD_ERR_INVALID, "need 999 >= t_start >= t_end >= 0");
    if (a->noise_mode != DD_NOISE_PHILOX && a->noise_mode != DD_NOISE_NONE)
        return ctx_fail(c, DD_ERR_INVALID, std::string(entry) + " generates noise on the device; for host noise drive dd_forward_early_exit");
    if ((behind_noise && (rc = behind_noise())) || (rc = check_image_seeds(c, a->noise_mode, a->B))) return rc;
    return (rc = stage_image_seeds(c, a->noise_mode, s, seeds)) ? rc : ensure_ee_ws(c, m);
}
}  // namespace

extern "C" {

int dd_scan_error(dd_ctx* c, const dd_scan_args* a, void* stream) { return scan_error(c, a, stream); }
int dd_scan_error_early_exit(dd_ctx* c, const dd_scan_exits_args* a, void* stream) { return scan_exits(c, a, stream); }

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
int dd_sample_affine_walk(dd_ctx* c, const dd_affine_sample_args* a, const dd_guidance* g, const dd_autoguidance* ag, const dd_known_region* kr,
                          const dd_walk* w, void* stream) {
    return sample_affine_walk(c, a, g, ag, kr, w, stream);
}
int dd_sample_affine_cached(dd_ctx* c, const dd_affine_sample_args* a, const dd_guidance* g, const dd_known_region* kr, const dd_block_cache* bc,
                            void* stream) {
    return sample_affine_cached(c, a, g, kr, bc, stream);
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

int dd_sample_early_exit(dd_ctx* c, const dd_ee_sample_args* a, void* stream) {
    const unsigned long long* seeds = nullptr;
    if (int rc = ee_sample_setup(c, a, "dd_sample_early_exit", (hipStream_t)stream, &seeds)) return rc;
    dd_model* m = a->model;
    // Two half-batch chains, as dd_sample: the samples are independent (every exit decision is per sample); the one quantity over the whole
    // batch -- the logged per-layer mean of the predicted errors, eesampler.py:70 -- becomes per-chain sums that one small launch joins
    // behind the loop, (chain 0 + chain 1) / B.  Heads and probes stay on each chain's own stream (measured: the 13 forks as parallel
    // branches of each chain's graph cost +0.9 ms per step -- 5.22 against 4.23 ms; profiles/r05/ab_round5.txt).
    const size_t tab = (size_t)1000 * m->cfg.depth;
    float* sums = m->ee_ws + ee_scratch_elems(m, m->cfg.max_batch);
    auto err_tab = [&](const Slice& sl) { return sl.chains == 1 || !a->err_dev ? a->err_dev : sums + sl.chain * tab; };
    Loop L{GRAPH_EARLY_EXIT, m, nullptr, switch_program(a->t_start - a->t_end + 1, -1), a->x_dev, a->y_dev, a->B, Mods{.seeds = seeds},
           a->use_graph != 0};
    L.set_state = [&](StepState* st, hipStream_t s) { return launch_set_state(st, a->t_start, (unsigned long long)a->seed, s); };
    L.key = [&](GraphKey& k, const Slice& sl) {
        k.noise = a->noise_mode; k.aux0 = err_tab(sl); k.aux1 = a->idx_dev; k.thr = a->threshold;
        if (sl.chains == 2 && sl.chain == 0) k.b0 = -1;     // (chain 0 of two -- not the whole batch's graph)
    };
    L.step = [&](dd_model* mm, const Chain& ch, const Slice& sl, bool, hipStream_t s) {
        return enqueue_ee_step(c, mm, ch, sl.x, sl.y, a->threshold, err_tab(sl), a->idx_dev, a->noise_mode, sl.B, s, sl.b0, a->B, sl.chains == 2,
                               sl.mods.seeds);
    };
    L.tail = [&](int chains, hipStream_t s) -> int {
        if (chains == 2 && a->err_dev) DD_HIP(c, launch_ee_mean_combine(sums, sums + tab, a->err_dev, m->cfg.depth, a->t_end, a->t_start, a->B, s));
        return DD_OK;
    };
    return run_loop(c, L, (hipStream_t)stream);
}

}  // extern "C"

namespace {
// The buffers of chain workspace ws that are live between the taps of block bi and its first launch, as image slabs: what a compaction in
// front of block bi has to move.  Read off the flags and the Handoff that Backbone itself reads (forward.hip):
//   x                              the residual stream (under hand.xfrag: its extra-token rows)
//   xfrag                          hand.xfrag: the patch rows of the residual stream
//   h | hfrag | qkv                where the launches in front left the block's norm1 (hand.h / hand.frag) or attn.qkv (hand.qkv)
//   xb                             an out-block whose skip_linear has not run: its x operand
//   skips[j], skipfrags[j]         every long-skip copy no skip_linear has consumed yet: j < bi (in- and mid-blocks); j < nb - bi, less the
//                                  one the previous block's fused launch consumed (hand.skip)
// ao / aofrag, hid, dec, mlp_partial and ytap are written and read inside one block or one taps stage: never live here.
int real_live_set(dd_ctx* c, const dd_model* m, const WsPtrs& ws, int bi, const Handoff& hand, RealSlabs& out) {
    const long long D = m->D, L = m->L, N = m->N, es = (long long)m->esize, nb = (long long)m->blocks.size();
    out.n = 0;
    int rc = DD_OK;
    auto add = [&](const void* p, long long bytes) {
        if (!p) return;
        if (out.n == EE_REAL_MAX_SLABS || bytes % 16 || (uintptr_t)p % 16) { rc = DD_ERR_UNSUPPORTED; return; }
        out.s[out.n++] = RealSlab{(char*)p, bytes};
    };
    add(ws.x, L * D * 4);
    if (hand.xfrag) add(ws.xfrag, N * D * 4);
    if (hand.h) add(ws.h, L * D * es);
    if (hand.frag) add(ws.hfrag, N * D * 2);
    if (hand.qkv) add(ws.qkv, 3 * D * (long long)make_head_major(m->L, m->H).Lp * es);
    if (bi > m->half_depth && !hand.skip) add(ws.xb, L * D * es);
    const long long unconsumed = bi <= m->half_depth ? bi : nb - bi - (hand.skip ? 1 : 0);
    for (long long j = 0; j < unconsumed; ++j) {
        add(ws.skips[j], L * D * es);
        if (m->frag_skip) add(ws.skipfrags[j], N * D * 2);
    }
    if (rc) return ctx_fail(c, rc, "real early exit: a per-image buffer of this model is no multiple of 16 bytes, or too many are live");
    return DD_OK;
}

// a chain's tables (RealTables) as one run of ints: rec [2 B] | moves [2 (B / 2 + 1)] | tab [B] | counts [2], an even number (rec and moves hold pairs)
size_t real_tab_ints(size_t B) { return (2 * B + 2 * (B / 2 + 1) + B + 2 + 1) / 2 * 2; }
// ... of chain k in the model's allocation (ensure_real_ws: both chains' runs, each sized for max_batch)
RealTables real_tables(const dd_model* m, int k) {
    const size_t B = (size_t)m->cfg.max_batch;
    int *rec = m->real_tabs + (size_t)k * real_tab_ints(B), *moves = rec + 2 * B, *tab = moves + 2 * (B / 2 + 1);
    return RealTables{tab, rec, tab + B, moves};
}
int ensure_real_ws(dd_ctx* c, dd_model* m) {
    if (!m->real_tabs) DD_HIP(c, hipMalloc((void**)&m->real_tabs, 2 * real_tab_ints((size_t)m->cfg.max_batch) * sizeof(int)));
    if (!m->real_counts_host) DD_HIP(c, hipHostMalloc((void**)&m->real_counts_host, 4 * sizeof(int), hipHostMallocDefault));
    for (hipEvent_t& e : m->real_ev)
        if (!e) DD_HIP(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return DD_OK;
}

// One chain of dd_sample_early_exit_real: its share of the batch, its scratch (ee_block: dd_sample_early_exit's block) and where it
// stands.  run() enqueues on the chain's stream until the chain is done or has to know a count: then the copy of the two counts and an
// event are enqueued behind the decision launch and run() returns, to be called again -- it waits on the event first.
struct RealChain {
    dd_ctx* c; dd_model* m; const dd_ee_sample_args* a;
    Chain ch; hipStream_t s;
    float* x; const int64_t* y; int B, b0;
    EeBlock blk;
    RealTables t; int* counts_host; hipEvent_t ev;
    const unsigned long long* seeds;
    int compact_every;
    int step = 0, layer = 0, Ba = 0;
    bool waiting = false, done = false;
    Handoff hand{};
    long long stats[3] = {0, 0, 0};
    double wait_ms = 0.0; long long waits = 0, bytes = 0;

    // (every stage is given the taps: a block's fused tail writes the y its successor's head reads only where the forward has taps)
    int stage(int kind) {
        RealStage r{kind, layer, kind == REAL_EMBED ? B : Ba, B};
        r.x_img = x; r.y = y; r.ee = &blk.taps; r.eps = blk.eps;
        return real_exit_stage(m, ch, r, hand, s);
    }
    int finish_step() {
        DD_HIP(c, launch_ee_real_step(x, blk.taps.outs, blk.eps, t, a->threshold, m->cfg.depth, ch.st, c->coef, B, m->cfg.in_chans, m->cfg.img_size, a->noise_mode, b0, seeds, s));
        layer = 0;
        done = ++step == a->t_start - a->t_end + 1;
        return DD_OK;
    }
    int run() {
        const int depth = m->cfg.depth;
        while (!done) {
            if (!waiting) {
                if (layer == 0) {
                    if (int rc = stage(REAL_EMBED)) return rc;
                    Ba = B;
                }
                if (int rc = stage(REAL_TAPS)) return rc;
                const bool compact = layer % compact_every == 0;
                DD_HIP(c, launch_ee_real_decide(blk.taps.cls + (size_t)layer * B, a->threshold, layer, depth, Ba, compact, t, a->idx_dev, a->B, b0, ch.st, s));
                if (compact) {
                    DD_HIP(c, hipMemcpyAsync(counts_host, t.counts, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
                    DD_HIP(c, hipEventRecord(ev, s));
                    waiting = true;
                    return DD_OK;
                }
            } else {
                const auto t0 = std::chrono::steady_clock::now();
                DD_HIP(c, hipEventSynchronize(ev));
                wait_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
                ++waits;
                waiting = false;
                const int keep = counts_host[0], moves = counts_host[1];
                if (keep < 0 || keep > Ba || moves < 0 || moves > Ba - keep) return ctx_fail(c, DD_ERR_HIP, "real early exit: the decision launch returned counts outside the batch");
                if (moves > 0 && keep > 0) {
                    RealSlabs slabs;
                    if (int rc = real_live_set(c, m, *ch.ws, layer, hand, slabs)) return rc;
                    DD_HIP(c, launch_ee_real_compact(t, moves, slabs, s));
                    stats[1] += moves; stats[2] += 1;
                    for (int i = 0; i < slabs.n; ++i) bytes += (long long)moves * slabs.s[i].bytes;
                }
                Ba = keep;
                if (Ba == 0) {       // every image of the chain has left: no further block, no output head
                    if (int rc = finish_step()) return rc;
                    continue;
                }
            }
            if (int rc = stage(REAL_BLOCK)) return rc;
            stats[0] += Ba;
            if (++layer == depth) {
                if (int rc = stage(REAL_HEAD)) return rc;
                if (int rc = finish_step()) return rc;
            }
        }
        return DD_OK;
    }
};
}  // namespace

extern "C" {

// dd_sample_early_exit with the exits taken.  Eager launches; the calling thread waits for each compaction layer's counts.
int dd_sample_early_exit_real(dd_ctx* c, const dd_ee_sample_args* a, const dd_ee_real* r, void* stream) {
    if (c && a && !r) return ctx_fail(c, DD_ERR_INVALID, "null dd_ee_real");
    hipStream_t s = (hipStream_t)stream;
    const unsigned long long* seeds = nullptr;
    int rc = ee_sample_setup(c, a, "dd_sample_early_exit_real", s, &seeds, [&]() -> int {
        if (a->err_dev) return ctx_fail(c, DD_ERR_INVALID, "dd_sample_early_exit_real: err_dev must be NULL (an image that has left has no predicted error at the layers behind its exit)");
        if (r->compact_every < 1) return ctx_fail(c, DD_ERR_INVALID, "dd_sample_early_exit_real: compact_every must be at least 1");
        return DD_OK;
    }, [&]() -> int {
        if (a->B > EE_REAL_MAX_SLOTS) return ctx_fail(c, DD_ERR_UNSUPPORTED, "dd_sample_early_exit_real takes at most 1024 images");
        return DD_OK;
    });
    if (rc) return rc;
    dd_model* m = a->model;
    if ((rc = ensure_real_ws(c, m))) return rc;
    for (long long& v : c->real_stats) v = 0;
    c->real_wait_ms = 0.0; c->real_waits = c->real_bytes = 0;
    // the chains of dd_sample_early_exit's policy (an eager loop here: no graph is asked for)
    const bool chained = use_chains(c, m, a->B, true);
    const int chains = chained ? 2 : 1, B0 = chained ? a->B / 2 : a->B;
    c->last_chains = chains;
    if (chained && (rc = ensure_chain_ws(c, m, s))) return rc;
    const size_t chw = (size_t)m->cfg.in_chans * m->cfg.img_size * m->cfg.img_size;
    for (int k = 0; k < chains; ++k) DD_HIP(c, launch_set_state(c->st[k], a->t_start, (unsigned long long)a->seed, s));
    ChainFork chain_fork{c, s, chained};
    if ((rc = chain_fork.fork())) return rc;
    DD_HIP(c, hipEventRecord(c->ev[0], s));
    RealChain rcs[2];
    for (int k = 0; k < chains; ++k) {
        const int b0 = k ? B0 : 0, Bk = k ? a->B - B0 : B0;
        rcs[k] = RealChain{c, m, a, Chain{&m->ws[k], c->st[k], c->num_cus, false}, k ? c->side : s,
                           a->x_dev + (size_t)b0 * chw, a->y_dev ? a->y_dev + b0 : nullptr, Bk, b0, ee_block(m, b0, Bk), real_tables(m, k),
                           m->real_counts_host + 2 * k, m->real_ev[k], seeds, r->compact_every};
    }
    // one host thread alternates the chains: one chain's blocks run while the other's counts travel
    for (bool busy = true; busy;) {
        busy = false;
        for (int k = 0; k < chains; ++k) {
            if (rcs[k].done) continue;
            if ((rc = rcs[k].run())) return rc;
            busy = busy || !rcs[k].done;
        }
    }
    for (int k = 0; k < chains; ++k) {
        for (int i = 0; i < 3; ++i) c->real_stats[i] += rcs[k].stats[i];
        c->real_wait_ms += rcs[k].wait_ms; c->real_waits += rcs[k].waits; c->real_bytes += rcs[k].bytes;
    }
    if ((rc = chain_fork.join())) return rc;
    DD_HIP(c, hipEventRecord(c->ev[1], s));
    DD_HIP(c, hipEventRecord(c->ev[2], s));
    return DD_OK;
}

int dd_dev_ee_real_stats(dd_ctx* c, long long out3[3]) {
    if (!c || !out3) return DD_ERR_INVALID;
    for (int i = 0; i < 3; ++i) out3[i] = c->real_stats[i];
    return DD_OK;
}
int dd_dev_ee_real_cost(dd_ctx* c, double* ms_out, long long* waits_out, long long* bytes_out) {
    if (!c || !ms_out || !waits_out || !bytes_out) return DD_ERR_INVALID;
    *ms_out = c->real_wait_ms; *waits_out = c->real_waits; *bytes_out = c->real_bytes;
    return DD_OK;
}
int dd_dev_ee_real_plan(const int* alive, int n, int* keep_out, int* n_moves_out, int* moves_src_dst) {
    if (!alive || n < 0 || !keep_out || !n_moves_out || !moves_src_dst) return DD_ERR_INVALID;
    *keep_out = real_exit_plan(alive, n, n_moves_out, moves_src_dst);
    return DD_OK;
}

long long dd_dev_graph_captures(dd_ctx* c) { return c ? c->graph_captures : -1; }
int dd_dev_last_sample_chains(dd_ctx* c) { return c ? c->last_chains : -1; }

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

}  // extern "C"
