// KL-VAE decode behind the C ABI: reference models/utils/autoencoder.py
//   FrozenAutoencoderKL.decode :486-490  =  z/scale -> post_quant_conv -> Decoder.forward :403-449
//   Decoder: conv_in, mid (ResnetBlock, AttnBlock, ResnetBlock), 4 up levels x 3 ResnetBlocks (+ nearest-2x Upsample
//   with conv), GroupNorm(32, eps 1e-6) + swish + conv_out.  ddconfig of get_autoencoder :503-516 (ch 128, mult 1,2,4,4).
// Activations are NHWC with an fp32 residual stream; every convolution is an explicit im2col (upsample folded into
// the gather) + one MFMA GEMM of gemm.hip with the bias / residual add fused in its epilogue.  The decode runs once per
// image (0.5 % of the FLOPs of 1000 sampling steps), so the design goal is correctness on parity-proven kernels.
// KL-VAE encode: FrozenAutoencoderKL.encode_moments / sample / encode :468-484  =  Encoder.forward :292-317
//   (conv_in, 4 down levels x 2 ResnetBlocks + Downsample behind levels 0-2, mid, GroupNorm + swish + conv_out) -> quant_conv ->
//   scale * (mean + std * eps).  Same conventions and the same ResnetBlock / AttnBlock definitions (Net below); built only when the
//   state_dict carried every encoder tensor.  Encode and decode of one object share one workspace: calls are ordered by the stream
//   they are given, and two calls on different streams must be ordered by the caller.
#include "../../include/duodiff.h"
#include "../../include/duodiff_dev.h"
#include "dd_internal.h"
#include "engine_state.h"
#include "host_arena.h"

#include <cmath>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <vector>

using namespace dd;


namespace {

struct ConvW { const void* w = nullptr; const float* b = nullptr; int cin = 0, cout = 0, k = 0, kpad = 0; };
struct NormW { const float* g = nullptr; const float* b = nullptr; int c = 0; };
struct ResW { NormW n1, n2; ConvW c1, c2, nin; };

struct HostT { std::vector<float> d; std::vector<int64_t> shape; };
struct GemmTap { dd_dev_vae_tap* t = nullptr; int seen = 0; };   // dd_dev_vae_trace: the caller's record, GEMM launches issued so far

}  // namespace

struct dd_vae {
    dd_ctx* ctx = nullptr;
    int max_chunk = 4, max_latent = 32;
    std::map<std::string, HostT> params;
    bool finalized = false;
    int prec = DD_PREC_BF16;
    size_t es = 2;
    char* warena = nullptr;
    char* ws = nullptr;
    // weights
    const float *pq_w = nullptr, *pq_b = nullptr;
    ConvW conv_in, conv_out, up_conv[4];
    ResW mid1, mid2, up[4][3];
    NormW attn_norm, norm_out;
    ConvW attn_q, attn_k, attn_v, attn_proj;
    // encoder weights (has_encoder: every one of expected_encoder() was set)
    bool has_encoder = false;
    const float *q_w = nullptr, *q_b = nullptr;
    ConvW e_conv_in, e_conv_out, e_down_conv[3];
    ResW e_down[4][2], e_mid1, e_mid2;
    NormW e_attn_norm, e_norm_out;
    ConvW e_attn_q, e_attn_k, e_attn_v, e_attn_proj;
    // workspace
    float *s0 = nullptr, *s1 = nullptr, *h1 = nullptr, *part = nullptr, *score = nullptr, *ao = nullptr, *z4 = nullptr;
    void *nb = nullptr, *col = nullptr, *q = nullptr, *kk = nullptr, *vt = nullptr, *pp = nullptr;
    GemmTap* tap = nullptr;     // set by dd_dev_vae_trace for the length of its call, null otherwise
};

namespace {

const int kCh = 128, kMult[4] = {1, 2, 4, 4};

#define VHIP(c, expr)                                                                  \
    do {                                                                               \
        hipError_t _e = (expr);                                                        \
        if (_e != hipSuccess) return ctx_fail((c), DD_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

// every decoder tensor the reference's state_dict holds, with its shape
std::map<std::string, std::vector<int64_t>> expected() {
    std::map<std::string, std::vector<int64_t>> m;
    auto conv = [&](const std::string& n, int co, int ci, int k) { m[n + ".weight"] = {co, ci, k, k}; m[n + ".bias"] = {co}; };
    auto norm = [&](const std::string& n, int c) { m[n + ".weight"] = {c}; m[n + ".bias"] = {c}; };
    auto res = [&](const std::string& n, int ci, int co) {
        norm(n + ".norm1", ci); conv(n + ".conv1", co, ci, 3); norm(n + ".norm2", co); conv(n + ".conv2", co, co, 3);
        if (ci != co) conv(n + ".nin_shortcut", co, ci, 1);
    };
    conv("post_quant_conv", 4, 4, 1);
    const int top = kCh * kMult[3];
    conv("decoder.conv_in", top, 4, 3);
    res("decoder.mid.block_1", top, top);
    norm("decoder.mid.attn_1.norm", top);
    for (const char* n : {"q", "k", "v", "proj_out"}) conv(std::string("decoder.mid.attn_1.") + n, top, top, 1);
    res("decoder.mid.block_2", top, top);
    int cin = top;
    for (int lv = 3; lv >= 0; --lv) {
        const int cout = kCh * kMult[lv];
        for (int j = 0; j < 3; ++j) { res("decoder.up." + std::to_string(lv) + ".block." + std::to_string(j), cin, cout); cin = cout; }
        if (lv != 0) conv("decoder.up." + std::to_string(lv) + ".upsample.conv", cin, cin, 3);
    }
    norm("decoder.norm_out", cin);
    conv("decoder.conv_out", 3, cin, 3);
    return m;
}

// every encode-side tensor of the reference's state_dict (encoder.* and quant_conv.*): 108 tensors, 34 163 664 values
std::map<std::string, std::vector<int64_t>> expected_encoder() {
    std::map<std::string, std::vector<int64_t>> m;
    auto conv = [&](const std::string& n, int co, int ci, int k) { m[n + ".weight"] = {co, ci, k, k}; m[n + ".bias"] = {co}; };
    auto norm = [&](const std::string& n, int c) { m[n + ".weight"] = {c}; m[n + ".bias"] = {c}; };
    auto res = [&](const std::string& n, int ci, int co) {
        norm(n + ".norm1", ci); conv(n + ".conv1", co, ci, 3); norm(n + ".norm2", co); conv(n + ".conv2", co, co, 3);
        if (ci != co) conv(n + ".nin_shortcut", co, ci, 1);
    };
    conv("encoder.conv_in", kCh, 3, 3);
    int cin = kCh;
    for (int lv = 0; lv < 4; ++lv) {
        const int cout = kCh * kMult[lv];
        for (int j = 0; j < 2; ++j) { res("encoder.down." + std::to_string(lv) + ".block." + std::to_string(j), cin, cout); cin = cout; }
        if (lv != 3) conv("encoder.down." + std::to_string(lv) + ".downsample.conv", cin, cin, 3);
    }
    res("encoder.mid.block_1", cin, cin);
    norm("encoder.mid.attn_1.norm", cin);
    for (const char* n : {"q", "k", "v", "proj_out"}) conv(std::string("encoder.mid.attn_1.") + n, cin, cin, 1);
    res("encoder.mid.block_2", cin, cin);
    norm("encoder.norm_out", cin);
    conv("encoder.conv_out", 8, cin, 3);
    conv("quant_conv", 8, 8, 1);
    return m;
}

// What both directions are made of, on one chunk of B images: the fp32 NHWC stream `cur` [B*H*H, Cc] (its twin `other`), the GEMM /
// im2col / GroupNorm wrappers, ResnetBlock and AttnBlock.  run_decode and run_encode hold the order of the layers only.
template <typename T>
struct Net {
    dd_vae* v;
    dd_ctx* c;
    hipStream_t s;
    int B, H, Cc = 0;
    T *nb, *col;
    float *cur, *other;

    Net(dd_vae* v_, int B_, int H_, hipStream_t s_)
        : v(v_), c(v_->ctx), s(s_), B(B_), H(H_), nb((T*)v_->nb), col((T*)v_->col), cur(v_->s0), other(v_->s1) {}

    // every GEMM of both directions is launched here; under dd_dev_vae_trace the chosen one is copied out around its launch
    int launch(const GemmArgs<T>& g, int epi) {
        if (v->tap) return traced(*v->tap, g, epi);
        VHIP(c, launch_gemm<T>(g, epi, s, c->num_cus));
        return DD_OK;
    }
    int traced(GemmTap& tp, const GemmArgs<T>& g, int epi) {
        dd_dev_vae_tap& t = *tp.t;
        const bool writes_x = epi == EPI_BIAS_RESID || epi == EPI_BIAS_SET, has_out = !writes_x && g.out;
        const size_t a_b = (size_t)g.M * g.K * sizeof(T), w_b = (size_t)g.N * g.K * sizeof(T), x_b = writes_x ? (size_t)g.M * g.N * 4 : 0,
                     o_b = has_out ? (size_t)g.M * g.ldo * sizeof(T) : 0;
        t.max_a_bytes = std::max(t.max_a_bytes, (long long)a_b); t.max_w_bytes = std::max(t.max_w_bytes, (long long)w_b);
        t.max_x_bytes = std::max(t.max_x_bytes, (long long)x_b); t.max_out_bytes = std::max(t.max_out_bytes, (long long)o_b);
        if (tp.seen++ != t.ordinal) {
            VHIP(c, launch_gemm<T>(g, epi, s, c->num_cus));
            return DD_OK;
        }
        if (g.lda != g.K || g.K1 != g.K || g.A2) return ctx_fail(c, DD_ERR_UNSUPPORTED, "dd_dev_vae_trace: a launch whose A is not one [M, K] matrix");
        if ((long long)a_b > t.a_bytes || (long long)w_b > t.w_bytes || (long long)g.N * 4 > t.bias_bytes || (long long)x_b > t.x_bytes || (long long)o_b > t.out_bytes || !t.A || !t.W ||
            !t.bias || (x_b && (!t.x_before || !t.x_after)) || (o_b && !t.out))
            return ctx_fail(c, DD_ERR_INVALID, "dd_dev_vae_trace: a host buffer is missing or too small for the chosen launch");
        t.M = g.M; t.N = g.N; t.K = g.K; t.epilogue = epi; t.ldo = has_out ? g.ldo : 0; t.has_bias = g.bias ? 1 : 0; t.tapped = 1;
        VHIP(c, hipStreamSynchronize(s));
        VHIP(c, hipMemcpy(t.A, g.A, a_b, hipMemcpyDeviceToHost));
        VHIP(c, hipMemcpy(t.W, g.W, w_b, hipMemcpyDeviceToHost));
        if (g.bias) VHIP(c, hipMemcpy(t.bias, g.bias, (size_t)g.N * 4, hipMemcpyDeviceToHost));
        if (x_b) VHIP(c, hipMemcpy(t.x_before, g.xres, x_b, hipMemcpyDeviceToHost));
        VHIP(c, launch_gemm<T>(g, epi, s, c->num_cus));
        VHIP(c, hipStreamSynchronize(s));
        if (x_b) VHIP(c, hipMemcpy(t.x_after, g.xres, x_b, hipMemcpyDeviceToHost));
        if (o_b) VHIP(c, hipMemcpy(t.out, g.out, o_b, hipMemcpyDeviceToHost));
        return DD_OK;
    }
    int gemm(const T* A, int M, int K, const ConvW& w, int epi, float* xres, T* o, int ldo) {
        return launch(GemmArgs<T>{A, nullptr, (const T*)w.w, w.b, xres, o, M, w.cout == 3 ? 4 : w.cout, K, K, K, 0, ldo}, epi);
    }
    // 3x3 conv of the T-typed NHWC image `src` (C channels at Hs x Hs, optionally upsampled 2x first)
    int conv3(const T* src, int Bn, int Hout, int C, int up, const ConvW& w, int epi, float* xres) {
        VHIP(c, launch_im2col3x3<T>(src, col, Bn, Hout, Hout, C, up, w.kpad, s));
        return gemm(col, Bn * Hout * Hout, w.kpad, w, epi, xres, nullptr, 0);
    }
    int gn(const float* x, const NormW& n, int Bn, int HW, int swish) {
        VHIP(c, launch_groupnorm<T>(x, v->part, n.g, n.b, nb, Bn, HW, n.c, swish, s));
        return DD_OK;
    }
    // ResnetBlock (autoencoder.py:121-136) on the fp32 stream `cur` [B*H*H, cin]
    int resnet(const ResW& r) {
        const int M = B * H * H, cin = r.c1.cin, cout = r.c1.cout;
        int rc;
        float* dst = cur;
        if (cin != cout) {   // x <- nin_shortcut(x) into the other stream buffer (1x1 conv on the raw stream)
            VHIP(c, launch_cast<T>(cur, (T*)v->q, (long long)M * cin, s));   // q buffer doubles as the raw-copy scratch
            if ((rc = gemm((const T*)v->q, M, cin, r.nin, EPI_BIAS_SET, other, nullptr, 0))) return rc;
            dst = other;
        }
        if ((rc = gn(cur, r.n1, B, H * H, 1))) return rc;
        if ((rc = conv3(nb, B, H, cin, 0, r.c1, EPI_BIAS_SET, v->h1))) return rc;
        if ((rc = gn(v->h1, r.n2, B, H * H, 1))) return rc;
        if ((rc = conv3(nb, B, H, cout, 0, r.c2, EPI_BIAS_RESID, dst))) return rc;     // x + h
        if (dst != cur) std::swap(cur, other);
        Cc = cout;
        return DD_OK;
    }
    // AttnBlock :155-185, single head over the H*H pixels of each image
    int attn(const NormW& norm, const ConvW& wq, const ConvW& wk, const ConvW& wv, const ConvW& wproj) {
        const int HW = H * H, C = Cc, M = B * HW;
        int rc;
        if ((rc = gn(cur, norm, B, HW, 0))) return rc;
        if ((rc = gemm(nb, M, C, wq, EPI_BIAS_STORE, nullptr, (T*)v->q, C))) return rc;
        if ((rc = gemm(nb, M, C, wk, EPI_BIAS_STORE, nullptr, (T*)v->kk, C))) return rc;
        for (int b = 0; b < B; ++b) {
            const T* hb = nb + (long long)b * HW * C;
            // V^T[c][tok] = Wv[c][:] . h[tok][:]  (bias of v is added after P.V: softmax rows sum to 1)
            GemmArgs<T> gv{(const T*)wv.w, nullptr, hb, nullptr, nullptr, (T*)v->vt, C, HW, C, C, C, 0, HW};
            if ((rc = launch(gv, EPI_STORE))) return rc;
            // S[i][j] = q_i . k_j  -> fp32
            GemmArgs<T> gs{(const T*)v->q + (long long)b * HW * C, nullptr, (const T*)v->kk + (long long)b * HW * C, nullptr,
                           v->score, nullptr, HW, HW, C, C, C, 0, 0};
            if ((rc = launch(gs, EPI_BIAS_SET))) return rc;
            VHIP(c, launch_softmax_rows<T>(v->score, (T*)v->pp, HW, HW, 1.0f / sqrtf((float)C), s));
            // O[i][c] = sum_j P[i][j] V^T[c][j] + b_v[c]
            GemmArgs<T> go{(const T*)v->pp, nullptr, (const T*)v->vt, wv.b, v->ao + (long long)b * HW * C, nullptr,
                           HW, C, HW, HW, HW, 0, 0};
            if ((rc = launch(go, EPI_BIAS_SET))) return rc;
        }
        VHIP(c, launch_cast<T>(v->ao, (T*)v->q, (long long)M * C, s));
        return gemm((const T*)v->q, M, C, wproj, EPI_BIAS_RESID, cur, nullptr, 0);  // x + proj_out(h_)
    }
};

template <typename T>
int run_decode(dd_vae* v, const float* z, float* out, int B, int HL, hipStream_t s) {
    Net<T> n(v, B, HL, s);
    dd_ctx* c = v->ctx;
    int rc;
    const int M0 = B * HL * HL;
    VHIP(c, launch_vae_input(z, v->pq_w, v->pq_b, 1.0f / 0.18215f, v->z4, B, HL * HL, s));               // :487-488
    VHIP(c, launch_im2col3x3_c4<T>(v->z4, n.col, B, HL, HL, v->conv_in.kpad, s));
    if ((rc = n.gemm(n.col, M0, v->conv_in.kpad, v->conv_in, EPI_BIAS_SET, n.cur, nullptr, 0))) return rc;   // conv_in :413
    n.Cc = v->conv_in.cout;
    if ((rc = n.resnet(v->mid1))) return rc;                                                               // :416
    if ((rc = n.attn(v->attn_norm, v->attn_q, v->attn_k, v->attn_v, v->attn_proj))) return rc;
    if ((rc = n.resnet(v->mid2))) return rc;                                                               // :418
    for (int lv = 3; lv >= 0; --lv) {                                                                      // :421-427
        for (int j = 0; j < 3; ++j)
            if ((rc = n.resnet(v->up[lv][j]))) return rc;
        if (lv != 0) {   // Upsample: nearest 2x + conv3x3 (:56-59); the upsample is folded into the im2col gather
            VHIP(c, launch_cast<T>(n.cur, n.nb, (long long)B * n.H * n.H * n.Cc, s));
            n.H *= 2;
            if ((rc = n.conv3(n.nb, B, n.H, n.Cc, 1, v->up_conv[lv], EPI_BIAS_SET, n.other))) return rc;
            std::swap(n.cur, n.other);
        }
    }
    if ((rc = n.gn(n.cur, v->norm_out, B, n.H * n.H, 1))) return rc;                                       // :433-434
    if ((rc = n.conv3(n.nb, B, n.H, n.Cc, 0, v->conv_out, EPI_BIAS_SET, v->h1))) return rc;                // :435  -> [M, 4]
    VHIP(c, launch_vae_output(v->h1, out, B, 3, n.H * n.H, 4, s));
    return DD_OK;
}

// x [B,3,HI,HI] -> moments [B,8,HI/8,HI/8] and / or z [B,4,HI/8,HI/8] (either may be null; eps null: the mode)
template <typename T>
int run_encode(dd_vae* v, const float* x, const float* eps, float* moments, float* z, int B, int HI, hipStream_t s) {
    Net<T> n(v, B, HI, s);
    dd_ctx* c = v->ctx;
    int rc;
    // the 4-channel input image lives in h1 (free until the first ResnetBlock), conv_out's [M, 8] rows too (as the decoder's [M, 4])
    VHIP(c, launch_vae_image(x, v->h1, B, HI * HI, s));
    VHIP(c, launch_im2col3x3_c4<T>(v->h1, n.col, B, HI, HI, v->e_conv_in.kpad, s));
    if ((rc = n.gemm(n.col, B * HI * HI, v->e_conv_in.kpad, v->e_conv_in, EPI_BIAS_SET, n.cur, nullptr, 0))) return rc;   // conv_in :297
    n.Cc = v->e_conv_in.cout;
    for (int lv = 0; lv < 4; ++lv) {                                                                       // :298-305
        for (int j = 0; j < 2; ++j)
            if ((rc = n.resnet(v->e_down[lv][j]))) return rc;
        if (lv != 3) {   // Downsample: pad (0,1,0,1) + conv3x3 stride 2 (:69-73); pad and stride are folded into the im2col gather
            const ConvW& w = v->e_down_conv[lv];
            VHIP(c, launch_cast<T>(n.cur, n.nb, (long long)B * n.H * n.H * n.Cc, s));
            n.H /= 2;
            VHIP(c, launch_im2col3x3_s2<T>(n.nb, n.col, B, n.H, n.H, n.Cc, w.kpad, s));
            if ((rc = n.gemm(n.col, B * n.H * n.H, w.kpad, w, EPI_BIAS_SET, n.other, nullptr, 0))) return rc;
            std::swap(n.cur, n.other);
        }
    }
    if ((rc = n.resnet(v->e_mid1))) return rc;                                                             // :309
    if ((rc = n.attn(v->e_attn_norm, v->e_attn_q, v->e_attn_k, v->e_attn_v, v->e_attn_proj))) return rc;
    if ((rc = n.resnet(v->e_mid2))) return rc;                                                             // :311
    if ((rc = n.gn(n.cur, v->e_norm_out, B, n.H * n.H, 1))) return rc;                                     // :314-315
    if ((rc = n.conv3(n.nb, B, n.H, n.Cc, 0, v->e_conv_out, EPI_BIAS_SET, v->h1))) return rc;              // :316  -> [M, 8]
    VHIP(c, launch_vae_moments(v->h1, v->q_w, v->q_b, eps, moments, z, B, n.H * n.H, s));                  // :470, :473-479
    return DD_OK;
}

}  // namespace

extern "C" {

int dd_vae_create(dd_ctx* c, int max_chunk, int max_latent, dd_vae** out) {
    if (!c || !out || max_chunk < 1 || max_latent < 1 || max_latent > 32) return DD_ERR_INVALID;
    dd_vae* v = new (std::nothrow) dd_vae();
    if (!v) return DD_ERR_NOMEM;
    v->ctx = c; v->max_chunk = max_chunk; v->max_latent = max_latent;
    *out = v;
    return DD_OK;
}

int dd_vae_set_param(dd_vae* v, const char* name, const float* data, const int64_t* shape, int ndim) {
    if (!v || !name || !data || !shape) return DD_ERR_INVALID;
    if (v->finalized) return ctx_fail(v->ctx, DD_ERR_STATE, "autoencoder already finalized");
    const std::string n(name);
    static const auto exp_dec = expected(), exp_enc = expected_encoder();
    const auto& exp = n.rfind("encoder.", 0) == 0 || n.rfind("quant_conv.", 0) == 0 ? exp_enc : exp_dec;
    auto it = exp.find(n);
    if (it == exp.end()) return ctx_fail(v->ctx, DD_ERR_NOT_FOUND, "unexpected key in autoencoder state_dict: " + n);
    std::vector<int64_t> got(shape, shape + ndim);
    if (got != it->second) return ctx_fail(v->ctx, DD_ERR_INVALID, "size mismatch for " + n);
    size_t cnt = 1;
    for (auto d : got) cnt *= (size_t)d;
    HostT& t = v->params[n];
    t.d.assign(data, data + cnt);
    t.shape = got;
    return DD_OK;
}

int dd_vae_finalize(dd_vae* v, int precision) {
    if (!v) return DD_ERR_INVALID;
    dd_ctx* c = v->ctx;
    if (v->finalized) return ctx_fail(c, DD_ERR_STATE, "autoencoder already finalized");
    if (precision != DD_PREC_BF16 && precision != DD_PREC_FP32) return ctx_fail(c, DD_ERR_INVALID, "unknown precision");
    for (auto& kv : expected())
        if (!v->params.count(kv.first)) return ctx_fail(c, DD_ERR_NOT_FOUND, "missing key in autoencoder state_dict: " + kv.first);
    VHIP(c, hipSetDevice(c->device));
    v->prec = precision;
    v->es = precision == DD_PREC_BF16 ? 2 : 4;
    const size_t es = v->es;
    const int kt = 128 / (int)es;   // GEMM k-tile in elements

    Arena w(es);
    auto P = [&](const std::string& n) -> const std::vector<float>& { return v->params[n].d; };
    // conv weight [Cout, Cin, k, k] -> GEMM matrix [Cout(+pad), (ky, kx, ci) padded to the k-tile]
    // (the encoder's conv_in: 3 input channels in the 4-channel stride of its input image, the fourth column of every tap zero)
    auto conv = [&](const std::string& n, ConvW& cw) {
        const auto& shp = v->params[n + ".weight"].shape;
        const int co = (int)shp[0], ci = (int)shp[1], k = (int)shp[2], cs = ci == 3 ? 4 : ci;
        const int K = k * k * cs, kpad = (K + kt - 1) / kt * kt, rows = co == 3 ? 4 : co;
        std::vector<float> m((size_t)rows * kpad, 0.f);
        const auto& wt = P(n + ".weight");
        for (int o = 0; o < co; ++o)
            for (int c2 = 0; c2 < ci; ++c2)
                for (int t = 0; t < k * k; ++t) m[(size_t)o * kpad + t * cs + c2] = wt[((size_t)o * ci + c2) * k * k + t];
        std::vector<float> b(rows, 0.f);
        std::memcpy(b.data(), P(n + ".bias").data(), co * 4);
        cw.cin = ci; cw.cout = co; cw.k = k; cw.kpad = kpad;
        w.mat(cw.w, m); w.f32(cw.b, b);
    };
    auto norm = [&](const std::string& n, NormW& nw) {
        nw.c = (int)P(n + ".weight").size();
        w.f32(nw.g, P(n + ".weight")); w.f32(nw.b, P(n + ".bias"));
    };
    auto res = [&](const std::string& n, ResW& r) {
        norm(n + ".norm1", r.n1); conv(n + ".conv1", r.c1); norm(n + ".norm2", r.n2); conv(n + ".conv2", r.c2);
        if (v->params.count(n + ".nin_shortcut.weight")) conv(n + ".nin_shortcut", r.nin);
    };
    w.f32(v->pq_w, P("post_quant_conv.weight")); w.f32(v->pq_b, P("post_quant_conv.bias"));
    conv("decoder.conv_in", v->conv_in);
    res("decoder.mid.block_1", v->mid1);
    norm("decoder.mid.attn_1.norm", v->attn_norm);
    conv("decoder.mid.attn_1.q", v->attn_q); conv("decoder.mid.attn_1.k", v->attn_k);
    conv("decoder.mid.attn_1.v", v->attn_v); conv("decoder.mid.attn_1.proj_out", v->attn_proj);
    res("decoder.mid.block_2", v->mid2);
    for (int lv = 3; lv >= 0; --lv) {
        for (int j = 0; j < 3; ++j) res("decoder.up." + std::to_string(lv) + ".block." + std::to_string(j), v->up[lv][j]);
        if (lv != 0) conv("decoder.up." + std::to_string(lv) + ".upsample.conv", v->up_conv[lv]);
    }
    norm("decoder.norm_out", v->norm_out);
    conv("decoder.conv_out", v->conv_out);
    v->has_encoder = true;      // iff every encode-side tensor was set; otherwise the object is decode-only
    for (auto& kv : expected_encoder())
        if (!v->params.count(kv.first)) { v->has_encoder = false; break; }
    if (v->has_encoder) {
        conv("encoder.conv_in", v->e_conv_in);
        for (int lv = 0; lv < 4; ++lv) {
            for (int j = 0; j < 2; ++j) res("encoder.down." + std::to_string(lv) + ".block." + std::to_string(j), v->e_down[lv][j]);
            if (lv != 3) conv("encoder.down." + std::to_string(lv) + ".downsample.conv", v->e_down_conv[lv]);
        }
        res("encoder.mid.block_1", v->e_mid1);
        norm("encoder.mid.attn_1.norm", v->e_attn_norm);
        conv("encoder.mid.attn_1.q", v->e_attn_q); conv("encoder.mid.attn_1.k", v->e_attn_k);
        conv("encoder.mid.attn_1.v", v->e_attn_v); conv("encoder.mid.attn_1.proj_out", v->e_attn_proj);
        res("encoder.mid.block_2", v->e_mid2);
        norm("encoder.norm_out", v->e_norm_out);
        conv("encoder.conv_out", v->e_conv_out);
        w.f32(v->q_w, P("quant_conv.weight")); w.f32(v->q_b, P("quant_conv.bias"));
    }
    VHIP(c, hipMalloc((void**)&v->warena, w.bytes()));
    VHIP(c, hipMemcpy(v->warena, w.image(), w.bytes(), hipMemcpyHostToDevice));
    w.bind(v->warena);

    // workspace for one chunk of images at the largest resolution (8 * latent); every buffer with the same slack behind it.  The encoder
    // fits the same buffers (its widest stream: 128 channels at full resolution, its widest im2col 1152 columns there; its 4-channel
    // input image and conv_out's [M, 8] rows live in h1)
    const size_t Bc = v->max_chunk, HWmax = (size_t)(8 * v->max_latent) * (8 * v->max_latent), slack = 512 * 4608 * 4;
    const size_t stream_elems = Bc * HWmax * 256;            // the upsample conv at the last level keeps 256 channels
    const size_t col_elems = Bc * HWmax * 2304;              // widest im2col: 256 channels at full resolution
    const size_t HWm = (size_t)v->max_latent * v->max_latent, Cm = 512;
    Arena a;
    auto buf = [&](auto*& field, size_t bytes) { a.space(field, bytes + slack); };
    buf(v->s0, stream_elems * 4); buf(v->s1, stream_elems * 4); buf(v->h1, stream_elems * 4);
    buf(v->nb, stream_elems * es); buf(v->col, col_elems * es);
    buf(v->part, (size_t)groupnorm_partials((int)Bc, (int)HWmax) * 4);
    buf(v->q, std::max(Bc * HWm * Cm, stream_elems) * es); buf(v->kk, Bc * HWm * Cm * es);
    buf(v->vt, Cm * HWm * es); buf(v->pp, HWm * HWm * es); buf(v->score, HWm * HWm * 4);
    buf(v->ao, Bc * HWm * Cm * 4); buf(v->z4, Bc * HWm * 4 * 4);
    VHIP(c, hipMalloc((void**)&v->ws, a.bytes()));
    VHIP(c, hipMemset(v->ws, 0, a.bytes()));
    VHIP(c, hipStreamSynchronize(nullptr));      // (ditto model.hip: ordered before any stream the decoder is later run on)
    a.bind(v->ws);
    for (auto& kv : v->params) std::vector<float>().swap(kv.second.d);
    v->finalized = true;
    return DD_OK;
}

int dd_vae_decode(dd_ctx* c, dd_vae* v, const float* z_dev, float* out_dev, int B, int latent_hw, void* stream) {
    if (!c || !v || v->ctx != c) return DD_ERR_INVALID;
    if (!v->finalized) return ctx_fail(c, DD_ERR_STATE, "dd_vae_finalize has not been called");
    if (!z_dev || !out_dev || B < 1) return ctx_fail(c, DD_ERR_INVALID, "null tensor or empty batch");
    if (latent_hw < 1 || latent_hw > v->max_latent) return ctx_fail(c, DD_ERR_INVALID, "latent size outside [1, max_latent]");
    if ((latent_hw * latent_hw) % 64) return ctx_fail(c, DD_ERR_UNSUPPORTED, "latent pixel count must be a multiple of 64 (attention k-tile)");
    hipStream_t s = (hipStream_t)stream;
    const long long zin = 4LL * latent_hw * latent_hw, zout = 3LL * 64 * latent_hw * latent_hw;
    for (int b0 = 0; b0 < B; b0 += v->max_chunk) {
        const int bn = std::min(v->max_chunk, B - b0);
        const int rc = v->prec == DD_PREC_BF16 ? run_decode<bf16_t>(v, z_dev + b0 * zin, out_dev + b0 * zout, bn, latent_hw, s)
                                               : run_decode<float>(v, z_dev + b0 * zin, out_dev + b0 * zout, bn, latent_hw, s);
        if (rc) return rc;
    }
    return DD_OK;
}

int dd_vae_has_encoder(const dd_vae* v) { return v && v->finalized && v->has_encoder ? 1 : 0; }

int dd_vae_encode(dd_ctx* c, dd_vae* v, const float* x_dev, const float* eps_dev, float* moments_dev, float* z_dev, int B, int image_hw,
                  void* stream) {
    if (!c || !v || v->ctx != c) return DD_ERR_INVALID;
    if (!v->finalized) return ctx_fail(c, DD_ERR_STATE, "dd_vae_finalize has not been called");
    if (!v->has_encoder) return ctx_fail(c, DD_ERR_UNSUPPORTED, "this autoencoder was loaded without the encoder (decode-only)");
    if (!x_dev || B < 1) return ctx_fail(c, DD_ERR_INVALID, "null tensor or empty batch");
    if (!moments_dev && !z_dev) return ctx_fail(c, DD_ERR_INVALID, "neither moments nor z is asked for");
    if (image_hw < 64 || image_hw % 64) return ctx_fail(c, DD_ERR_UNSUPPORTED, "image size must be a multiple of 64 (latent pixel count a multiple of 64: attention k-tile)");
    if (image_hw > 8 * v->max_latent) return ctx_fail(c, DD_ERR_INVALID, "image size above 8 * max_latent");
    hipStream_t s = (hipStream_t)stream;
    const int hl = image_hw / 8;
    const long long xin = 3LL * image_hw * image_hw, per = 4LL * hl * hl;
    for (int b0 = 0; b0 < B; b0 += v->max_chunk) {
        const int bn = std::min(v->max_chunk, B - b0);
        const float* x = x_dev + b0 * xin;
        const float* e = eps_dev ? eps_dev + b0 * per : nullptr;
        float* mo = moments_dev ? moments_dev + b0 * 2 * per : nullptr;
        float* z = z_dev ? z_dev + b0 * per : nullptr;
        const int rc = v->prec == DD_PREC_BF16 ? run_encode<bf16_t>(v, x, e, mo, z, bn, image_hw, s) : run_encode<float>(v, x, e, mo, z, bn, image_hw, s);
        if (rc) return rc;
    }
    return DD_OK;
}

int dd_vae_sample(dd_ctx* c, const float* moments_dev, const float* eps_dev, float* z_dev, int B, int latent_hw, void* stream) {
    if (!c) return DD_ERR_INVALID;
    if (!moments_dev || !z_dev || B < 1 || latent_hw < 1) return ctx_fail(c, DD_ERR_INVALID, "null tensor, empty batch or empty image");
    VHIP(c, launch_vae_sample(moments_dev, eps_dev, z_dev, B, latent_hw * latent_hw, (hipStream_t)stream));
    return DD_OK;
}

int dd_dev_vae_trace(dd_ctx* c, dd_vae* v, int encode, const float* in_dev, float* out_dev, int B, int hw, dd_dev_vae_tap* tap, void* stream) {
    if (!c || !v || v->ctx != c || !tap) return DD_ERR_INVALID;
    if (!v->finalized) return ctx_fail(c, DD_ERR_STATE, "dd_vae_finalize has not been called");
    if (encode && !v->has_encoder) return ctx_fail(c, DD_ERR_UNSUPPORTED, "this autoencoder was loaded without the encoder (decode-only)");
    const int hl = encode ? hw / 8 : hw;
    if (!in_dev || !out_dev || B < 1 || B > v->max_chunk || hl < 1 || hl > v->max_latent || (encode && hw % 8) || (hl * hl) % 64)
        return ctx_fail(c, DD_ERR_INVALID, "dd_dev_vae_trace: one chunk of images (B <= max_chunk) at a size dd_vae_decode / dd_vae_encode accepts");
    hipStream_t s = (hipStream_t)stream;
    GemmTap tp;
    tp.t = tap;
    tap->tapped = 0; tap->launches = 0;
    tap->max_a_bytes = tap->max_w_bytes = tap->max_x_bytes = tap->max_out_bytes = 0;
    v->tap = &tp;
    const bool bf = v->prec == DD_PREC_BF16;
    const int rc = encode ? (bf ? run_encode<bf16_t>(v, in_dev, nullptr, out_dev, nullptr, B, hw, s) : run_encode<float>(v, in_dev, nullptr, out_dev, nullptr, B, hw, s))
                          : (bf ? run_decode<bf16_t>(v, in_dev, out_dev, B, hw, s) : run_decode<float>(v, in_dev, out_dev, B, hw, s));
    v->tap = nullptr;
    tap->launches = tp.seen;
    return rc;
}

void dd_vae_destroy(dd_vae* v) {
    if (!v) return;
    if (v->warena) (void)hipFree(v->warena);
    if (v->ws) (void)hipFree(v->ws);
    delete v;
}

}  // extern "C"
