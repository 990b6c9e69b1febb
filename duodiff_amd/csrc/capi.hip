// extern "C" surface of libduodiff.so (include/duodiff.h), the part that takes no model: the context, the stateless step kernels' entry points
// and the development switches.  The model, the forward and the sampling loops are model.hip, forward.hip and loops.hip; all four share
// engine_state.h.  This unit carries the build id.
#include "../../include/duodiff.h"
#include "../../include/duodiff_dev.h"
#include "engine_state.h"

#include <cstdio>
#include <cstring>
#include <new>
#include <string>

using namespace dd;

// ==========================================================================================
extern "C" {

int dd_abi_version(void) { return DD_ABI_VERSION; }

#ifndef DD_BUILD_ID
#define DD_BUILD_ID "unknown"
#endif
const char* dd_build_id(void) { return DD_BUILD_ID; }

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
    ok = ok && init_kernel_tables() == hipSuccess;
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
    for (hipGraphExec_t g : c->jump_graph) if (g) (void)hipGraphExecDestroy(g);
    for (StepState* st : c->st) if (st) (void)hipFree(st);
    if (c->coef) (void)hipFree(c->coef);
    c->x_stage.release(); c->y_stage.release(); c->h_stage.release(); c->k_stage.release(); c->m_stage.release();
    c->atab.release(); c->htab.release(); c->ktab.release(); c->seeds_stage.release();
    c->stab.release(); c->scan_ws.release();
    for (auto& e : c->ev) if (e) (void)hipEventDestroy(e);
    delete c;
}

const char* dd_last_error(dd_ctx* c) { return c ? c->err.c_str() : "null context"; }

int dd_sync(dd_ctx* c, void* stream) {
    if (!c) return DD_ERR_INVALID;
    DD_HIP(c, hipStreamSynchronize((hipStream_t)stream));
    return DD_OK;
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

int dd_jump_step(dd_ctx* c, const float* x_dev, const float* z_dev, float ja, float jc, float* out_dev, int64_t n, void* stream) {
    if (!c) return DD_ERR_INVALID;
    if (!x_dev || !out_dev || n < 0) return ctx_fail(c, DD_ERR_INVALID, "null tensor");
    if (n == 0) return DD_OK;
    DD_HIP(c, launch_jump_step(x_dev, z_dev, out_dev, ja, jc, (long long)n, (hipStream_t)stream));
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

int dd_set_image_seeds(dd_ctx* c, const uint64_t* seeds_dev, int n) {
    if (!c) return DD_ERR_INVALID;
    if (n < 0 || (seeds_dev == nullptr) != (n == 0)) return ctx_fail(c, DD_ERR_INVALID, "dd_set_image_seeds: n seeds on the device, or NULL and 0 to clear");
    c->seeds_user = seeds_dev;
    c->seeds_n = n;
    return DD_OK;
}

int dd_noise_images(dd_ctx* c, uint64_t seed, const uint64_t* seeds_dev, int counter, float* out_dev, int B, int C, int S, void* stream) {
    if (!c) return DD_ERR_INVALID;
    if (!out_dev) return ctx_fail(c, DD_ERR_INVALID, "null tensor");
    if (B < 0 || C < 1 || C > 4 || S < 1 || S > 32768) return ctx_fail(c, DD_ERR_INVALID, "bad image shape: B >= 0, C in 1..4, S in 1..32768");
    if (counter < 0) return ctx_fail(c, DD_ERR_INVALID, "counter must not be negative");
    if (B == 0) return DD_OK;
    const hipError_t e = launch_noise_images(out_dev, (const unsigned long long*)seeds_dev, (unsigned long long)seed, counter, B, C, S, (hipStream_t)stream);
    if (e == hipErrorInvalidValue) return ctx_fail(c, DD_ERR_INVALID, "dd_noise_images: a batch this launch cannot cover");
    DD_HIP(c, e);
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

int dd_dev_kernel_table(int index, char family[32], int key[4], int* block, int* lds_max) {
    if (index < 0 || !family || !key || !block || !lds_max) return DD_ERR_INVALID;
    for (const KernelFamily& f : kernel_families())
        for (int i = 0; const KernelInfo* e = f.at(i); ++i, --index)
            if (index == 0) {
                std::snprintf(family, 32, "%s", f.name);
                std::memcpy(key, e->key.data(), sizeof(e->key));
                *block = e->block;
                *lds_max = e->lds_max;
                return 0;
            }
    return 1;
}

int dd_dev_kernel_supported(int predicate, const int args[6]) {
    if (!args) return DD_ERR_INVALID;
    EmbedArgs ea{};
    ea.P = args[0]; ea.C = args[1]; ea.D = args[2]; ea.S = args[3]; ea.L = args[4]; ea.extras = args[5];
    size_t lds = 0;
    switch (predicate) {
        case DD_DEV_SUP_MLP_FUSED: return mlp_fused_supported(args[0], args[1]);
        case DD_DEV_SUP_HEAD_DEC: return head_dec_supported(args[0], args[1]);
        case DD_DEV_SUP_HEAD_DEC_PROBE: return head_dec_probe_supported(args[0]);
        case DD_DEV_SUP_QKV_ATTENTION: return qkv_attention_supported(args[0], args[1], args[2], args[3]);
        case DD_DEV_SUP_ROWLIN: return rowlin_supported(args[0], args[1]);
        case DD_DEV_SUP_EMBED_MFMA: return embed_mfma_ok(ea, lds);
        case DD_DEV_SUP_EMBED_LN: return embed_ln_supported(ea);
    }
    return DD_ERR_INVALID;
}

int dd_set_num_cus(dd_ctx* c, int n) {
    if (!c) return DD_ERR_INVALID;
    if (n < 8) return ctx_fail(c, DD_ERR_INVALID, "need at least 8 CUs");
    c->num_cus = n / 8 * 8;      // the persistent kernels deal tiles to workgroups in groups of 8 (one per XCD)
    return DD_OK;
}

}  // extern "C"
