// The single-kernel development entry points of include/duodiff_dev.h (dd_dev_mlp, dd_dev_block_tail, dd_dev_block_tail_frag, dd_dev_qkv_attention, dd_dev_qkv_attention_rows, dd_dev_qkv_attention_frag, dd_dev_v_identity, dd_dev_v_copy, dd_dev_head_dec, dd_dev_gemm,
// dd_dev_rowlin, dd_dev_attention, dd_dev_attention_long, dd_dev_layernorm, dd_dev_embed, dd_dev_time_mlp, dd_dev_vae_gather, dd_dev_groupnorm, dd_dev_softmax_rows, dd_dev_vae_input, dd_dev_vae_output, dd_dev_vae_moments, dd_dev_cast, dd_dev_ee_probe, dd_dev_ee_probe_reduce, dd_dev_ee_attn_probe, dd_dev_final, dd_dev_scan_diffuse, dd_dev_scan_error, dd_dev_scan_exits_error): test scaffolding, not product.  Each one owns its host operands, device buffers, canaries and
// downloads, and nothing of the launch: the weight images come from finalize's packers and the launch arguments from the model's builders (launch_args.h:
// dd_dev_mlp and dd_dev_block_tail* run block_tail_plan / block_tail_finish exactly as Backbone::block_tail does), then `iters` further launch sequences
// are timed.  Buffers, transfers, timing and HIP errors go through one DevScope (dev_scope.h); of the context it reads num_cus and dev_flags (engine_state.h).
#include "../../include/duodiff.h"
#include "../../include/duodiff_dev.h"
#include "engine_state.h"
#include "launch_args.h"

#include <cstring>
#include <vector>

using namespace dd;

extern "C" {

int dd_dev_mlp(dd_ctx* c, int M, int D, int hidden, int extras, const float* x_host, const float* w1, const float* b1, const float* w2,
               const float* b2, float* xres_host, unsigned short* out_host, const float* ln_in, const float* ln_out,
               unsigned short* ln_out_host, int iters, void* stream, float* ms_out, const float* ao_host, const float* wproj,
               const float* bproj, const float* skip_host, const float* wskip, const float* bskip, const float* wqkv,
               unsigned short* qkv_out_host) {
    const bool proj = ao_host && wproj && bproj;
    const bool skp = skip_host && wskip && bskip;
    const bool qk = wqkv && qkv_out_host;
    if (qk && (!proj || !ln_out || (hidden / 32) % 2)) return DD_ERR_INVALID;   // the qkv phases ride on the proj-fused launch, behind norm1
    if (proj && (!ln_in || D % 128)) return DD_ERR_INVALID;   // the projection rides in the LayerNorm-in kernel only
    if (skp && (!proj || !ln_out || !ln_out_host || (hidden / 32) % 2)) return DD_ERR_INVALID;   // the skip phases ride on the proj-fused launch and end in norm1
    if (!c || !x_host || !w1 || !b1 || !w2 || !b2 || !xres_host || M < 1 || iters < 0 || extras < 0 || (extras > 0 && M % (1 + extras))) return DD_ERR_INVALID;
    if (!mlp_fused_supported(D, hidden)) return ctx_fail(c, DD_ERR_UNSUPPORTED, "fused MLP: D in {64,128,256,512}, hidden % 64 == 0");
    hipStream_t s = (hipStream_t)stream;
    const size_t Mp = (size_t)round_up(M, 256), row_bytes = Mp * D * 2;      // (every bf16 row buffer: Mp rows, zero padding)
    const TailImage t = pack_tail_image(D, hidden, proj ? wproj : nullptr, w1, b1, w2, ln_in != nullptr, skp ? wskip : nullptr, qk ? wqkv : nullptr);
    std::vector<float> xr(Mp * D, 0.f);
    std::memcpy(xr.data(), xres_host, (size_t)M * D * 4);
    // extras > 0: the M rows are `M / (1 + extras)` images of one patch token each (drives the hidden-split path);
    // extras == 0: one image of M patch tokens (main tiles only)
    const int B = extras > 0 ? M / (1 + extras) : 1, n_patches = extras > 0 ? 1 : M;
    DevScope dev(c);
    MlpFusedArgs a{};
    a.X = dev.upload(bf16_rows(x_host, M, D, Mp, 0).data(), row_bytes);
    a.wimg = (const char*)dev.upload(t.img.data(), t.img.size() * 2);
    a.b1p = dev.upload(t.b1p.data(), (size_t)hidden * 4); a.b2 = dev.upload(b2, (size_t)D * 4);
    a.xres = dev.upload(xr.data(), xr.size() * 4);
    bf16_t* dO = dev.filled<bf16_t>(row_bytes, 0);
    a.out = out_host || skp ? dO : nullptr;      // (a SKIP launch: y of the extra-token rows travels through the bf16 copy)
    // ln_in / ln_out: [2, D] gamma then beta of the LayerNorm fused into the prologue / epilogue (or NULL)
    bf16_t* dH = dev.filled<bf16_t>(row_bytes, 0);
    if (ln_in) { a.ln_in_g = dev.upload(ln_in, (size_t)2 * D * 4); a.ln_in_b = a.ln_in_g + D; }
    if (ln_out && ln_out_host) { a.ln_out_g = dev.upload(ln_out, (size_t)2 * D * 4); a.ln_out_b = a.ln_out_g + D; a.ln_out = dH; }
    if (proj) { a.ao = dev.upload(bf16_rows(ao_host, M, D, Mp, 0).data(), row_bytes); a.bproj = dev.upload(bproj, (size_t)D * 4); }
    if (skp) { a.skip = dev.upload(bf16_rows(skip_host, M, D, Mp, 0).data(), row_bytes); a.bskip = dev.upload(bskip, (size_t)D * 4); }
    // head-major qkv of the rows as images of n_patches + extras tokens (HeadMajor, dd_internal.h): [images][3 D / 64 units][Lp][64]
    const size_t qkv_elems = qk ? (size_t)B * 3 * D * make_head_major(n_patches + extras, D / 64).Lp : 0;
    if (qk) { a.qkv_out = dev.filled<bf16_t>(qkv_elems * 2, 0); a.qkv_dump = dev.alloc<bf16_t>(16384); }
    block_tail_plan(a, B, n_patches, extras, D, D / 64, hidden, false);
    if (c->dev_flags & DD_DEV_MLP_EXTRAS_ONLY) { a.tiles_main = 0; a.n_main = 0; }   // time the hidden-split workgroups alone
    const size_t part = (size_t)a.tiles_left * a.groups * 128 * D * sizeof(float);
    a.partial = part ? dev.alloc<float>(part) : nullptr;
    auto once = [&]() -> hipError_t {
        const hipError_t e = launch_mlp_fused(a, D, s);
        return e == hipSuccess ? block_tail_finish(a, D, s) : e;
    };
    DEV_HIP(dev, once());
    DEV_HIP(dev, hipStreamSynchronize(s));
    if (qk) dev.download(qkv_out_host, a.qkv_out, qkv_elems * 2);
    dev.download(xres_host, a.xres, (size_t)M * D * 4);
    if (out_host) dev.download(out_host, dO, (size_t)M * D * 2);
    if (a.ln_out) dev.download(ln_out_host, dH, (size_t)M * D * 2);
    DEV_HIP(dev, time_launches(s, iters, once, ms_out));
    return dev.status();
}

}  // extern "C"

// dd_dev_block_tail and dd_dev_block_tail_frag: the second adds the patch rows' hand-offs in fragment order (all null: the first)
static int block_tail_run(dd_ctx* c, int B, int n_patches, int extras, int D, int hidden, int last, int poison, const float* h_host,
                          const float* w1, const float* b1, const float* w2, const float* b2, const float* ln_in, const float* ao_host,
                          const float* wproj, const float* bproj, const float* ln_out, const float* skip_host, const float* wskip,
                          const float* bskip, const float* wqkv, float* xres_host, unsigned short* out_host, unsigned short* ln_out_host,
                          unsigned short* frag_host, float* tap_host, unsigned short* qkv_host, float* slab_host, int slab_rows, int* plan_out,
                          int iters, void* stream, float* ms_out, const unsigned short* ao_frag_host, const unsigned short* skip_frag_host,
                          const float* xin_frag_host, unsigned short* out_frag_host, float* xout_frag_host) {
    const bool proj = ao_host && wproj && bproj;
    const bool skp = skip_host && wskip && bskip;
    const bool qk = wqkv && qkv_host;
    const bool lnout = ln_out && ln_out_host;
    const bool frag = frag_host != nullptr, tap = tap_host != nullptr;
    if (!c || B < 1 || n_patches < 1 || extras < 0 || extras > 2 || D < 1 || hidden < 1 || !w1 || !b1 || !w2 || !b2 || !xres_host || iters < 0 ||
        poison < 0 || poison > 255 || slab_rows < 0 || (slab_rows > 0) != (slab_host != nullptr) || (ln_in != nullptr) == (h_host != nullptr))
        return DD_ERR_INVALID;
    if ((proj && !ln_in) || (lnout && !ln_in) || (frag && !lnout) || (skp && (!proj || !lnout || !out_host)) || (tap && !skp) ||
        (qk && (!proj || !lnout)) || (last && (!proj || lnout || skp || qk)))
        return DD_ERR_INVALID;
    if (!mlp_fused_supported(D, hidden)) return ctx_fail(c, DD_ERR_UNSUPPORTED, "fused MLP: D in {64,128,256,512}, hidden % 64 == 0");
    if (frag && skp && extras > 0 && D != 512) return ctx_fail(c, DD_ERR_UNSUPPORTED, "block tail: skip rows without their LayerNorm at D = 512 only");
    if ((ao_frag_host && !proj) || (skip_frag_host && !skp) || (out_frag_host && !out_host)) return DD_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int L = extras + n_patches, M = B * L;
    // the fragment-order buffers hold the B n_patches patch rows; the output ones carry 8 canary rows (0xFF bytes) in front and behind.  The patch
    // rows of the row-major device buffer a fragment operand stands in for hold `poison` bytes: the main tiles must not read them
    const size_t pe = (size_t)B * n_patches * D, guard = (size_t)8 * D;
    auto rows_patch_poisoned = [&](const float* src) {
        std::vector<unsigned short> r = bf16_rows(src, M, D, (size_t)round_up(M, 256) + 8, (unsigned char)poison);
        for (int b = 0; b < B; ++b) std::memset(r.data() + ((size_t)b * L + extras) * D, poison, (size_t)n_patches * D * 2);
        return r;
    };
    const size_t Mo = (size_t)round_up(M, 256) + 8, n16 = Mo * D * 2, n32 = Mo * D * 4;
    const TailImage t = pack_tail_image(D, hidden, proj ? wproj : nullptr, w1, b1, w2, ln_in != nullptr, skp ? wskip : nullptr, qk ? wqkv : nullptr);
    DevScope dev(c);
    MlpFusedArgs a{};
    // operands: Mo rows, the rows [M, Mo) hold `poison` bytes; X = nullptr in LayerNorm-in mode, as in the model
    a.X = h_host ? dev.upload(bf16_rows(h_host, M, D, Mo, (unsigned char)poison).data(), n16) : nullptr;
    a.wimg = (const char*)dev.upload(t.img.data(), t.img.size() * 2);
    a.b1p = dev.upload(t.b1p.data(), (size_t)hidden * 4); a.b2 = dev.upload(b2, (size_t)D * 4);
    if (ln_in) { a.ln_in_g = dev.upload(ln_in, (size_t)2 * D * 4); a.ln_in_b = a.ln_in_g + D; }
    if (xin_frag_host) {      // the patch rows come from the fragment buffer: their row-major copies hold `poison`
        std::vector<float> xr(xres_host, xres_host + Mo * D);
        for (int b = 0; b < B; ++b) std::memset(xr.data() + ((size_t)b * L + extras) * D, poison, (size_t)n_patches * D * 4);
        a.xres = dev.upload(xr.data(), n32);
        a.x_in_frag = dev.upload(xin_frag_host, pe * 4);
    } else {
        a.xres = dev.upload(xres_host, n32);
    }
    if (xout_frag_host) a.x_out_frag = dev.filled<float>((pe + 2 * guard) * 4, 0xFF) + guard;
    if (out_frag_host) a.out_frag = dev.filled<bf16_t>((pe + 2 * guard) * 2, 0xFF) + guard;
    a.out = out_host ? dev.filled<bf16_t>(n16, 0xFF) : nullptr;
    if (proj) {
        a.ao = dev.upload((ao_frag_host ? rows_patch_poisoned(ao_host) : bf16_rows(ao_host, M, D, Mo, (unsigned char)poison)).data(), n16);
        a.bproj = dev.upload(bproj, (size_t)D * 4);
        if (ao_frag_host) a.ao_frag = dev.upload(ao_frag_host, pe * 2);
    }
    if (skp) {
        a.skip = dev.upload((skip_frag_host ? rows_patch_poisoned(skip_host) : bf16_rows(skip_host, M, D, Mo, (unsigned char)poison)).data(), n16);
        if (skip_frag_host) a.skip_frag = dev.upload(skip_frag_host, pe * 2);
        if (tap) a.y_tap = dev.filled<float>(n32, 0xFF);
        a.bskip = dev.upload(bskip, (size_t)D * 4);
    }
    if (lnout) { a.ln_out_g = dev.upload(ln_out, (size_t)2 * D * 4); a.ln_out_b = a.ln_out_g + D; a.ln_out = dev.filled<bf16_t>(n16, 0xFF); }
    if (frag) a.ln_out_frag = dev.filled<bf16_t>(n16, 0xFF);
    const size_t qkv_elems = qk ? ((size_t)B * 3 * (D / 64) * make_head_major(L, D / 64).Lp + 64) * 64 : 0;
    if (qk) { a.qkv_out = dev.filled<bf16_t>(qkv_elems * 2, 0xFF); a.qkv_dump = dev.alloc<bf16_t>(16384); }
    block_tail_plan(a, B, n_patches, extras, D, D / 64, hidden, last != 0);
    if ((size_t)slab_rows < (size_t)a.tiles_left * a.groups * a.prows) return DD_ERR_INVALID;
    if (plan_out) { plan_out[0] = a.tiles_main; plan_out[1] = a.tiles_left; plan_out[2] = a.groups; plan_out[3] = a.prows; }
    a.partial = slab_rows ? dev.filled<float>((size_t)slab_rows * D * 4, poison) : nullptr;
    auto once = [&]() -> hipError_t {
        const hipError_t e = launch_mlp_fused(a, D, s);
        return e == hipSuccess ? block_tail_finish(a, D, s) : e;
    };
    const hipError_t first = dev.ok() ? launch_mlp_fused(a, D, s) : hipSuccess;
    if (first == hipErrorInvalidValue) return ctx_fail(c, DD_ERR_UNSUPPORTED, "block tail: a combination of modes launch_mlp_fused refuses");      // (refused before any launch)
    DEV_HIP(dev, first);
    DEV_HIP(dev, block_tail_finish(a, D, s));
    DEV_HIP(dev, hipStreamSynchronize(s));
    dev.download(xres_host, a.xres, n32);
    if (out_host) dev.download(out_host, a.out, n16);
    if (lnout) dev.download(ln_out_host, a.ln_out, n16);
    if (frag) dev.download(frag_host, a.ln_out_frag, n16);
    if (tap) dev.download(tap_host, a.y_tap, n32);
    if (qk) dev.download(qkv_host, a.qkv_out, qkv_elems * 2);
    if (slab_rows) dev.download(slab_host, a.partial, (size_t)slab_rows * D * 4);
    if (xout_frag_host) dev.download(xout_frag_host, a.x_out_frag - guard, (pe + 2 * guard) * 4);
    if (out_frag_host) dev.download(out_frag_host, a.out_frag - guard, (pe + 2 * guard) * 2);
    DEV_HIP(dev, time_launches(s, iters, once, ms_out));
    return dev.status();
}

extern "C" {

int dd_dev_block_tail(dd_ctx* c, int B, int n_patches, int extras, int D, int hidden, int last, int poison, const float* h_host,
                      const float* w1, const float* b1, const float* w2, const float* b2, const float* ln_in, const float* ao_host,
                      const float* wproj, const float* bproj, const float* ln_out, const float* skip_host, const float* wskip,
                      const float* bskip, const float* wqkv, float* xres_host, unsigned short* out_host, unsigned short* ln_out_host,
                      unsigned short* frag_host, float* tap_host, unsigned short* qkv_host, float* slab_host, int slab_rows, int* plan_out,
                      int iters, void* stream, float* ms_out) {
    return block_tail_run(c, B, n_patches, extras, D, hidden, last, poison, h_host, w1, b1, w2, b2, ln_in, ao_host, wproj, bproj, ln_out, skip_host, wskip,
                          bskip, wqkv, xres_host, out_host, ln_out_host, frag_host, tap_host, qkv_host, slab_host, slab_rows, plan_out, iters, stream,
                          ms_out, nullptr, nullptr, nullptr, nullptr, nullptr);
}

int dd_dev_block_tail_frag(dd_ctx* c, int B, int n_patches, int extras, int D, int hidden, int last, int poison, const float* h_host,
                           const float* w1, const float* b1, const float* w2, const float* b2, const float* ln_in, const float* ao_host,
                           const float* wproj, const float* bproj, const float* ln_out, const float* skip_host, const float* wskip,
                           const float* bskip, const float* wqkv, float* xres_host, unsigned short* out_host, unsigned short* ln_out_host,
                           unsigned short* frag_host, float* tap_host, unsigned short* qkv_host, float* slab_host, int slab_rows, int* plan_out,
                           int iters, void* stream, float* ms_out, const unsigned short* ao_frag_host, const unsigned short* skip_frag_host,
                           const float* xin_frag_host, unsigned short* out_frag_host, float* xout_frag_host) {
    return block_tail_run(c, B, n_patches, extras, D, hidden, last, poison, h_host, w1, b1, w2, b2, ln_in, ao_host, wproj, bproj, ln_out, skip_host, wskip,
                          bskip, wqkv, xres_host, out_host, ln_out_host, frag_host, tap_host, qkv_host, slab_host, slab_rows, plan_out, iters, stream,
                          ms_out, ao_frag_host, skip_frag_host, xin_frag_host, out_frag_host, xout_frag_host);
}

}  // extern "C"

// The head-major qkv image of B images (HeadMajor: B 3 H units of Lp rows, 64 trailing rows) as launch_attention / launch_v_copy read it, from
// row(u, l), the 64 floats of token l of unit u: 0xFF bytes (NaN) everywhere, then the rows l < L only -- the pad rows [L, Lp) of every unit, which the
// qkv Linear never writes, and the trailing rows stay NaN
template <typename Row>
static std::vector<unsigned char> head_major_image(bool bf, int B, int L, int H, Row row) {
    const size_t units = (size_t)B * 3 * H, Lp = (size_t)make_head_major(L, H).Lp;
    std::vector<unsigned char> img((units * Lp + 64) * 64 * (bf ? 2 : 4), 0xFF);
    for (size_t u = 0; u < units; ++u)
        for (int l = 0; l < L; ++l) {
            const float* r = row(u, l);
            const size_t at = (u * Lp + l) * 64;
            if (bf) for (int d = 0; d < 64; ++d) reinterpret_cast<unsigned short*>(img.data())[at + d] = host_f2bf(r[d]);
            else std::memcpy(img.data() + at * 4, r, 64 * 4);
        }
    return img;
}

// The device operands of launch_qkv_attention / launch_v_identity on B images of 256 patch tokens behind `extras` extra tokens, from the norm1 rows
// h_host [B L, D]: the patch rows in fragment order (what the fused block tail writes: MlpFusedArgs::ln_out_frag), the weight image, and the
// extra-token rows row-major -- norm1 as bf16 (hx), or (xres_host) the fp32 residual stream the kernel normalises itself with ln.  The patch rows of
// either, which the kernel must never read, hold 0xFF bytes (NaN)
struct QkvOperands {
    const bf16_t *hf, *img, *hx = nullptr;
    const float *xres = nullptr, *ln_g = nullptr, *ln_b = nullptr, *bias = nullptr;
};
static QkvOperands qkv_operands(DevScope& dev, int B, int L, int H, int extras, const float* h_host, const float* wqkv, const float* bqkv,
                                const float* xres_host, const float* ln) {
    const int D = 64 * H;
    const size_t M = (size_t)B * L;
    std::vector<unsigned short> hb = bf16_rows(h_host, M, D, M, 0);
    std::vector<unsigned short> hf((size_t)B * 256 * D), img((size_t)3 * D * D);
    for (int b = 0; b < B; ++b)
        for (int n = 0; n < 256; ++n)
            for (int k = 0; k < D; ++k)
                hf[((((size_t)b * 8 + n / 32) * (D / 16) + k / 16) * 64 + (n % 32) + 32 * ((k % 16) / 8)) * 8 + k % 8] = hb[((size_t)b * L + extras + n) * D + k];
    qkv_attention_pack(D, H, wqkv, host_f2bf, img.data());
    QkvOperands q;
    q.hf = (const bf16_t*)dev.upload(hf.data(), hf.size() * 2);
    q.img = (const bf16_t*)dev.upload(img.data(), img.size() * 2);
    if (xres_host) {
        std::vector<float> xr(M * D);
        std::memset(xr.data(), 0xFF, xr.size() * 4);
        for (int b = 0; b < B; ++b) std::memcpy(xr.data() + (size_t)b * L * D, xres_host + (size_t)b * L * D, (size_t)extras * D * 4);
        q.xres = dev.upload(xr.data(), xr.size() * 4);
        q.ln_g = dev.upload(ln, (size_t)2 * D * 4); q.ln_b = q.ln_g + D;
    } else {
        for (int b = 0; b < B; ++b) std::memset(hb.data() + ((size_t)b * L + extras) * D, 0xFF, (size_t)256 * D * 2);
        q.hx = (const bf16_t*)dev.upload(hb.data(), hb.size() * 2);
    }
    if (bqkv) q.bias = dev.upload(bqkv, (size_t)3 * D * 4);
    return q;
}

// dd_dev_qkv_attention_rows, dd_dev_qkv_attention_frag (out_frag_host non-null: the patch rows' output in fragment order) and dd_dev_v_identity
// (identity: launch_v_identity on the same operands, the extra-token rows from the residual stream)
static int qkv_attention_run(dd_ctx* c, int B, int L, int H, int extras, const float* h_host, const float* wqkv, const float* bqkv,
                             const float* xres_host, const float* ln, unsigned short* out_host, unsigned short* out_frag_host, bool identity, int iters,
                             void* stream, float* ms_out) {
    if (!c || !h_host || !wqkv || !out_host || (identity ? !xres_host || !ln : xres_host && !ln) || B < 1 || iters < 0) return DD_ERR_INVALID;
    const int D = 64 * H;
    if (!qkv_attention_supported(D, H, L, extras))
        return ctx_fail(c, DD_ERR_UNSUPPORTED, std::string(identity ? "v_identity" : "qkv_attention") + ": D = 512 / 768 / 1024, L = 256 + 1 or 2 extra tokens only");
    hipStream_t s = (hipStream_t)stream;
    const size_t M = (size_t)B * L;
    DevScope dev(c);
    const QkvOperands q = qkv_operands(dev, B, L, H, extras, h_host, wqkv, bqkv, xres_host, ln);
    bf16_t* dO = dev.filled<bf16_t>((M + 8) * D * 2, 0xFF);      // 8 canary rows behind the output
    const size_t pe = (size_t)B * 256 * D, guard = (size_t)8 * D;          // the fragment-order output: 8 canary rows in front and behind
    bf16_t* dF = out_frag_host ? dev.filled<bf16_t>((pe + 2 * guard) * 2, 0xFF) + guard : nullptr;
    auto once = [&]() {
        return identity ? launch_v_identity(q.hf, q.img, q.bias, q.xres, q.ln_g, q.ln_b, dO, B, L, H, D, extras, s)
                        : launch_qkv_attention(q.hf, q.img, q.bias, q.hx, q.xres, q.ln_g, q.ln_b, dO, B, L, H, D, extras, s, dF);
    };
    DEV_HIP(dev, once());
    DEV_HIP(dev, hipStreamSynchronize(s));
    dev.download(out_host, dO, (M + 8) * D * 2);
    if (out_frag_host) dev.download(out_frag_host, dF - guard, (pe + 2 * guard) * 2);
    DEV_HIP(dev, time_launches(s, iters, once, ms_out));
    return dev.status();
}

// dd_dev_attention (launch_attention) and dd_dev_attention_long (long_kernel: launch_attention_long) on the same operands
static int attention_run(dd_ctx* c, int precision, int B, int L, int H, const float* q, const float* k, const float* v, void* out_host,
                         bool long_kernel, int iters, void* stream, float* ms_out) {
    const bool bf = precision == DD_PREC_BF16;
    if (!c || (!bf && precision != DD_PREC_FP32) || B < 1 || L < 1 || H < 1 || !q || !k || !v || !out_host || iters < 0) return DD_ERR_INVALID;
    const char* bound = long_kernel ? "attention_long: 1 <= L <= 4098, heads of 64" : "attention: 1 <= L <= 288, heads of 64";
    if (L > (long_kernel ? kMaxLongL : 288)) return ctx_fail(c, DD_ERR_UNSUPPORTED, bound);      // (before the host image of such an L is built)
    hipStream_t s = (hipStream_t)stream;
    const int D = 64 * H;
    const size_t esz = bf ? 2 : 4, out_elems = ((size_t)B * L + 8) * D;
    const float* src[3] = {q, k, v};      // unit u = (b 3 + j) H + head: q | k | v [B, H, L, 64]
    const std::vector<unsigned char> img = head_major_image(bf, B, L, H, [&](size_t u, int l) {
        return src[u / H % 3] + ((u / (3 * (size_t)H) * H + u % H) * L + l) * 64;
    });
    DevScope dev(c);
    const void* dQ = dev.upload(img.data(), img.size());
    void* dO = dev.filled(out_elems * esz, 0xFF);
    auto once = [&]() {
        if (long_kernel) return bf ? launch_attention_long<bf16_t>((const bf16_t*)dQ, (bf16_t*)dO, B, L, H, D, s) : launch_attention_long<float>((const float*)dQ, (float*)dO, B, L, H, D, s);
        return bf ? launch_attention<bf16_t>((const bf16_t*)dQ, (bf16_t*)dO, B, L, H, D, s) : launch_attention<float>((const float*)dQ, (float*)dO, B, L, H, D, s);
    };
    const hipError_t first = dev.ok() ? once() : hipSuccess;
    if (first == hipErrorInvalidValue) return ctx_fail(c, DD_ERR_UNSUPPORTED, bound);      // (refused before any launch)
    DEV_HIP(dev, first);
    DEV_HIP(dev, hipStreamSynchronize(s));
    dev.download(out_host, dO, out_elems * esz);
    DEV_HIP(dev, time_launches(s, iters, once, ms_out));
    return dev.status();
}

extern "C" {

int dd_dev_qkv_attention_rows(dd_ctx* c, int B, int L, int H, int extras, const float* h_host, const float* wqkv, const float* bqkv,
                              const float* xres_host, const float* ln, unsigned short* out_host, int iters, void* stream, float* ms_out) {
    return qkv_attention_run(c, B, L, H, extras, h_host, wqkv, bqkv, xres_host, ln, out_host, nullptr, false, iters, stream, ms_out);
}

int dd_dev_qkv_attention_frag(dd_ctx* c, int B, int L, int H, int extras, const float* h_host, const float* wqkv, const float* bqkv,
                              const float* xres_host, const float* ln, unsigned short* out_host, unsigned short* out_frag_host, int iters,
                              void* stream, float* ms_out) {
    if (!out_frag_host) return DD_ERR_INVALID;
    return qkv_attention_run(c, B, L, H, extras, h_host, wqkv, bqkv, xres_host, ln, out_host, out_frag_host, false, iters, stream, ms_out);
}

int dd_dev_v_identity(dd_ctx* c, int B, int L, int H, int extras, const float* h_host, const float* wqkv, const float* bqkv,
                      const float* xres_host, const float* ln, unsigned short* out_host, int iters, void* stream, float* ms_out) {
    return qkv_attention_run(c, B, L, H, extras, h_host, wqkv, bqkv, xres_host, ln, out_host, nullptr, true, iters, stream, ms_out);
}

int dd_dev_v_copy(dd_ctx* c, int precision, int B, int L, int H, const float* qkv_host, void* out_host, int iters, void* stream, float* ms_out) {
    const bool bf = precision == DD_PREC_BF16;
    if (!c || (!bf && precision != DD_PREC_FP32) || B < 1 || L < 1 || H < 1 || !qkv_host || !out_host || iters < 0) return DD_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int D = 64 * H;
    const size_t esz = bf ? 2 : 4, out_elems = ((size_t)B * L + 8) * D;
    const std::vector<unsigned char> img = head_major_image(bf, B, L, H, [&](size_t u, int l) { return qkv_host + (u * L + l) * 64; });
    DevScope dev(c);
    const void* dQ = dev.upload(img.data(), img.size());
    void* dO = dev.filled(out_elems * esz, 0xFF);
    auto once = [&]() {
        return bf ? launch_v_copy<bf16_t>((const bf16_t*)dQ, (bf16_t*)dO, B, L, H, D, s) : launch_v_copy<float>((const float*)dQ, (float*)dO, B, L, H, D, s);
    };
    const hipError_t first = dev.ok() ? once() : hipSuccess;
    if (first == hipErrorInvalidValue) return ctx_fail(c, DD_ERR_UNSUPPORTED, "v_copy: 1 <= L <= 288, heads of 64");      // (refused before any launch)
    DEV_HIP(dev, first);
    DEV_HIP(dev, hipStreamSynchronize(s));
    dev.download(out_host, dO, out_elems * esz);
    DEV_HIP(dev, time_launches(s, iters, once, ms_out));
    return dev.status();
}

int dd_dev_qkv_attention(dd_ctx* c, int B, int L, int H, int extras, const float* h_host, const float* wqkv, const float* bqkv,
                         unsigned short* out_host, int iters, void* stream, float* ms_out) {
    if (!out_host) return DD_ERR_INVALID;
    std::vector<unsigned short> whole(B > 0 && L > 0 && H > 0 ? ((size_t)B * L + 8) * 64 * H : 0);      // (a refused shape does not touch it)
    const int st = dd_dev_qkv_attention_rows(c, B, L, H, extras, h_host, wqkv, bqkv, nullptr, nullptr, whole.data(), iters, stream, ms_out);
    if (st == DD_OK) std::memcpy(out_host, whole.data(), (size_t)B * L * 64 * H * 2);
    return st;
}

int dd_dev_head_dec(dd_ctx* c, int M, int D, int pd, int tok_l, int tok_e, const float* x_host, const float* norm_g, const float* norm_b,
                    const float* wdec, const float* bdec, float* dec_host, const float* probe_w, const float* probe_b, float* srow_host,
                    int split, int iters, void* stream, float* ms_out) {
    if (!c || !x_host || !norm_g || !norm_b || !wdec || !bdec || !dec_host || M < 1 || iters < 0) return DD_ERR_INVALID;
    if (!head_dec_supported(D, pd)) return ctx_fail(c, DD_ERR_UNSUPPORTED, "head_dec: D in {256, 512, 768, 1024}, pd % 4 == 0, pd <= 64");
    const bool probe = probe_w && probe_b && srow_host;
    if (probe && !head_dec_probe_supported(D)) return ctx_fail(c, DD_ERR_UNSUPPORTED, "head_dec with the probe: D in {256, 512}");
    hipStream_t s = (hipStream_t)stream;
    if (split && !head_dec_probe_supported(D)) return ctx_fail(c, DD_ERR_UNSUPPORTED, "head_dec as a split-bf16 product: D in {256, 512}");
    const HeadImage hi = pack_head_image(D, pd, wdec, bdec, norm_g, norm_b, split != 0);
    DevScope dev(c);
    const float* dX = dev.upload(x_host, (size_t)M * D * 4);
    // split: the packed image in wg's place, and the constants whose second half are the row sums of hi + lo (HeadDecArgs::split)
    const float* dW = split ? (const float*)dev.upload(hi.wsplit.data(), hi.wsplit.size() * 2) : dev.upload(hi.wg.data(), hi.wg.size() * 4);
    const float* dC = dev.upload((split ? hi.dcs : hi.dc).data(), hi.dc.size() * 4);
    float* dO = dev.filled<float>((size_t)M * pd * 4, 0xFF);      // NaN: rows the launch does not decode stay recognisable
    HeadDecArgs ha{dX, dW, dC, dO, M, pd, tok_l, tok_e};
    ha.split = split ? 1 : 0;
    if (probe) {
        ha.pw_base = dev.upload(probe_w, (size_t)D * 4); ha.pb_base = dev.upload(probe_b, 4);
        ha.srow = dev.filled<float>((size_t)M * 4, 0xFF);     // (probe row 0: t_mul = add = 0, the step state is not read)
    }
    auto once = [&]() { return launch_head_dec(ha, D, c->num_cus, s); };
    DEV_HIP(dev, once());
    DEV_HIP(dev, hipStreamSynchronize(s));
    dev.download(dec_host, dO, (size_t)M * pd * 4);
    if (probe) dev.download(srow_host, ha.srow, (size_t)M * 4);
    DEV_HIP(dev, time_launches(s, iters, once, ms_out));
    return dev.status();
}

int dd_dev_gemm(dd_ctx* c, int precision, int M, int N, int K, int K1, const float* A, const float* A2, const float* W, const float* bias,
                int epilogue, int tile128, int hm_L, int hm_H, int splits, int resid, const float* ln, int tok_l, int tok_e,
                float* xres_host, void* out_host, int ldo, unsigned short* h_host, unsigned short* frag_host, float* slab_host,
                int num_cus, int iters, void* stream, float* ms_out) {
    const bool bf = precision == DD_PREC_BF16;
    if (K1 == 0) K1 = K;
    const int KT = bf ? 64 : 32;
    if (!c || (!bf && precision != DD_PREC_FP32) || M < 1 || N < 4 || N % 4 || K < KT || K % KT || K1 < KT || K1 > K || K1 % KT || !A || !W ||
        (K1 < K && !A2) || ldo < N || ldo % (bf ? 8 : 4) || iters < 0 || num_cus < 0 || (num_cus > 0 && num_cus < 8) || tile128 < -1 || tile128 > 1)
        return DD_ERR_INVALID;
    if (splits > 0 && (!bf || splits < 2 || !bias || hm_L || (ln && !h_host) || (frag_host && (!ln || tok_l <= tok_e))))
        return ctx_fail(c, DD_ERR_INVALID, "split-K: bf16, splits >= 2, bias, no head-major map; LayerNorm output needs h (and frag tok_l > tok_e)");
    if (splits == 0 && (epilogue < EPI_STORE || epilogue > EPI_BIAS_STORE || ((epilogue == EPI_BIAS_RESID || epilogue == EPI_BIAS_SET) && !xres_host) ||
                        (epilogue != EPI_STORE && epilogue != EPI_BIAS_SET && !bias) || (hm_L && (hm_H < 1 || M % hm_L || !out_host))))
        return DD_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const size_t esz = bf ? 2 : 4, Mo = (size_t)round_up(M, 256) + 8;
    const HeadMajor hm = hm_L ? make_head_major(hm_L, hm_H) : HeadMajor{};
    const size_t out_elems = hm_L ? ((size_t)(M / hm_L) * 3 * hm_H * hm.Lp + 64) * 64 : Mo * ldo;
    const int lda = K1, lda2 = K - K1;
    DevScope dev(c);
    // operands as the kernel reads them: bf16 (or fp32) rows; A / A2 padded to Mo rows of 0xFF bytes (NaN: a row read past M shows up as one)
    auto operand = [&](const float* src, size_t rows, size_t cols, size_t alloc_rows) -> const void* {
        if (bf) return dev.upload(bf16_rows(src, rows, cols, alloc_rows, 0xFF).data(), alloc_rows * cols * 2);
        std::vector<unsigned char> v(alloc_rows * cols * 4, 0xFF);
        std::memcpy(v.data(), src, rows * cols * 4);
        return dev.upload(v.data(), v.size());
    };
    const void* dA = operand(A, M, lda, Mo);
    const void* dA2 = K1 < K ? operand(A2, M, lda2, Mo) : nullptr;
    const void* dW = operand(W, N, K, N);
    const float* dBias = bias ? dev.upload(bias, (size_t)N * 4) : nullptr;
    // every output buffer: canary bytes (0xFF) everywhere, or the caller's bytes (xres, canary rows included), returned whole
    float* dX = xres_host ? dev.upload(xres_host, Mo * N * 4) : nullptr;
    void* dO = out_host ? dev.filled(out_elems * esz, 0xFF) : nullptr;
    const size_t slab_elems = (size_t)(splits > 0 ? splits : 0) * Mo * N;
    float *dP = nullptr, *dLn = nullptr;
    bf16_t *dH = nullptr, *dF = nullptr;
    if (splits > 0) {
        if (!dX) dX = dev.filled<float>(Mo * N * 4, 0xFF);      // (resid == 0: x = the Linear; the caller may not want it back)
        dP = dev.filled<float>(slab_elems * 4, 0xFF);
        if (ln) dLn = dev.upload(ln, (size_t)2 * N * 4);
        if (h_host) dH = dev.filled<bf16_t>(Mo * N * 2, 0xFF);
        if (frag_host) dF = dev.filled<bf16_t>(Mo * N * 2, 0xFF);
    }
    auto once = [&]() -> hipError_t {
        if (!bf) {
            GemmArgs<float> g{(const float*)dA, (const float*)dA2, (const float*)dW, dBias, dX, (float*)dO, M, N, K, K1, lda,
                              K1 < K ? lda2 : lda, ldo};
            g.hm = hm;
            return launch_gemm<float>(g, epilogue, s, num_cus ? num_cus : c->num_cus);
        }
        GemmArgs<bf16_t> g{(const bf16_t*)dA, (const bf16_t*)dA2, (const bf16_t*)dW, dBias, dX, (bf16_t*)dO, M, N, K, K1, lda,
                           K1 < K ? lda2 : lda, ldo};
        g.hm = hm;
        g.tile128 = tile128;
        if (splits == 0) return launch_gemm<bf16_t>(g, epilogue, s, num_cus ? num_cus : c->num_cus);
        g.partial = dP; g.splits = splits;
        hipError_t e = launch_gemm_splitk(g, s, num_cus ? num_cus : c->num_cus);
        if (e != hipSuccess) return e;
        const float* lg = ln ? dLn : nullptr;
        return launch_reduce_ln(splitk_reduce_args(g, resid, lg, lg ? lg + N : nullptr, dH, dF, tok_l, tok_e), N, s);
    };
    DEV_HIP(dev, once());
    DEV_HIP(dev, hipStreamSynchronize(s));
    if (xres_host) dev.download(xres_host, dX, Mo * N * 4);
    if (out_host) dev.download(out_host, dO, out_elems * esz);
    if (h_host && dH) dev.download(h_host, dH, Mo * N * 2);
    if (frag_host && dF) dev.download(frag_host, dF, Mo * N * 2);
    if (slab_host && dP) dev.download(slab_host, dP, slab_elems * 4);
    DEV_HIP(dev, time_launches(s, iters, once, ms_out));
    return dev.status();
}

int dd_dev_rowlin(dd_ctx* c, int B, int n_patches, int extras, int K, int k_split, int set_x, const float* A, const float* A2, const float* W,
                  const float* bias, const float* ln, float* xres_host, unsigned short* x_copy_host, unsigned short* h_host, int frag,
                  int iters, void* stream, float* ms_out) {
    constexpr int D = 768;
    const bool planned = n_patches > 0;
    if (!c || B < 1 || n_patches < 0 || extras < 0 || (!planned && extras) || !A || !W || !bias || !xres_host || iters < 0 ||
        (k_split && (2 * k_split != K || !A2)) || (h_host && !ln))
        return DD_ERR_INVALID;
    if (!rowlin_supported(D, K)) return ctx_fail(c, DD_ERR_UNSUPPORTED, "rowlin: K % 64 == 0, K >= 192");
    hipStream_t s = (hipStream_t)stream;
    const int M = planned ? B * (n_patches + extras) : B;
    const size_t Mo = (size_t)round_up(M, 256) + 8;
    const int lda = k_split ? k_split : K;
    std::vector<unsigned short> img((size_t)K * D);
    rowlin_pack(K, W, host_f2bf, img.data());      // as finalize packs the model's rowlin images
    DevScope dev(c);
    // A / A2 padded to Mo rows of 0xFF bytes; every output buffer: canary bytes (0xFF) everywhere, or the caller's bytes (xres)
    const bf16_t* dA = dev.upload(bf16_rows(A, M, lda, Mo, 0xFF).data(), Mo * lda * 2);
    const bf16_t* dA2 = k_split ? dev.upload(bf16_rows(A2, M, lda, Mo, 0xFF).data(), Mo * lda * 2) : nullptr;
    const bf16_t* dW = dev.upload(img.data(), img.size() * 2);
    const float* dBias = dev.upload(bias, (size_t)D * 4);
    float* dX = dev.upload(xres_host, Mo * D * 4);
    bf16_t* dC = x_copy_host ? dev.filled<bf16_t>(Mo * D * 2, 0xFF) : nullptr;
    const float* lg = ln ? dev.upload(ln, (size_t)2 * D * 4) : nullptr;
    bf16_t* dH = h_host ? dev.filled<bf16_t>(Mo * D * 2, 0xFF) : nullptr;
    const size_t part = planned ? rowlin_partial_bytes(B, extras, K) : 0;
    float* dP = part ? dev.filled<float>(part, 0xFF) : nullptr;
    GemmArgs<bf16_t> g{dA, dA2, nullptr, dBias, dX, dC, M, D, K, k_split ? k_split : K, lda, lda, D};
    const RowLinArgs ra = rowlin_args(g, !set_x, (const char*)dW, dP, lg, lg ? lg + D : nullptr, frag ? nullptr : dH, frag ? dH : nullptr,
                                      B, n_patches, extras);
    const MlpFusedArgs fr = rowlin_reduce_args(ra);
    auto once = [&]() -> hipError_t {
        hipError_t e = launch_rowlin(ra, s);
        return e == hipSuccess ? launch_mlp_reduce(fr, D, s) : e;
    };
    DEV_HIP(dev, once());
    DEV_HIP(dev, hipStreamSynchronize(s));
    dev.download(xres_host, dX, Mo * D * 4);
    if (x_copy_host) dev.download(x_copy_host, dC, Mo * D * 2);
    if (h_host) dev.download(h_host, dH, Mo * D * 2);
    DEV_HIP(dev, time_launches(s, iters, once, ms_out));
    return dev.status();
}

int dd_dev_attention(dd_ctx* c, int precision, int B, int L, int H, const float* q, const float* k, const float* v, void* out_host,
                     int iters, void* stream, float* ms_out) {
    return attention_run(c, precision, B, L, H, q, k, v, out_host, false, iters, stream, ms_out);
}

int dd_dev_attention_long(dd_ctx* c, int precision, int B, int L, int H, const float* q, const float* k, const float* v, void* out_host,
                          int iters, void* stream, float* ms_out) {
    return attention_run(c, precision, B, L, H, q, k, v, out_host, true, iters, stream, ms_out);
}

int dd_dev_layernorm(dd_ctx* c, int precision, int rows, int D, const float* x_host, const float* gamma_beta, void* out_host,
                     unsigned short* frag_host, int tok_l, int tok_e, int iters, void* stream, float* ms_out) {
    const bool bf = precision == DD_PREC_BF16;
    if (!c || (!bf && precision != DD_PREC_FP32) || rows < 1 || D < 1 || !x_host || !gamma_beta || !out_host || iters < 0) return DD_ERR_INVALID;
    if (frag_host && !bf) return ctx_fail(c, DD_ERR_UNSUPPORTED, "layernorm: fragment order is a bf16 output");
    hipStream_t s = (hipStream_t)stream;
    const size_t n_out = ((size_t)rows + 8) * D;
    DevScope dev(c);
    const float* dX = dev.upload(x_host, (size_t)rows * D * 4);
    const float* dG = dev.upload(gamma_beta, (size_t)2 * D * 4);
    void* dO = dev.filled(n_out * (bf ? 2 : 4), 0xFF);
    bf16_t* dF = frag_host ? dev.filled<bf16_t>(n_out * 2, 0xFF) : nullptr;
    auto once = [&]() {
        if (frag_host) return launch_layernorm_frag(dX, dG, dG + D, (bf16_t*)dO, dF, rows, D, tok_l, tok_e, s);
        return bf ? launch_layernorm<bf16_t>(dX, dG, dG + D, (bf16_t*)dO, rows, D, s) : launch_layernorm<float>(dX, dG, dG + D, (float*)dO, rows, D, s);
    };
    const hipError_t first = dev.ok() ? once() : hipSuccess;
    if (first == hipErrorInvalidValue)      // (refused before any launch)
        return ctx_fail(c, DD_ERR_UNSUPPORTED, "layernorm: D % 64 == 0, D <= 1024; fragment order: D % 256 == 0, (tok_l - tok_e) % 32 == 0, rows % tok_l == 0");
    DEV_HIP(dev, first);
    DEV_HIP(dev, hipStreamSynchronize(s));
    dev.download(out_host, dO, n_out * (bf ? 2 : 4));
    if (frag_host) dev.download(frag_host, dF, n_out * 2);
    DEV_HIP(dev, time_launches(s, iters, once, ms_out));
    return dev.status();
}

int dd_dev_cache_extrapolate(dd_ctx* c, int precision, int rows, int D, const void* last_host, const void* prev_host, int op, float w, int table,
                             void* out_host, int iters, void* stream, float* ms_out) {
    const bool bf = precision == DD_PREC_BF16;
    if (!c || (!bf && precision != DD_PREC_FP32) || rows < 1 || rows > (1 << 24) || D < 64 || D % 64 || D > 4096 || !last_host || !prev_host ||
        !out_host || op < 0 || op > 2 || iters < 0)
        return DD_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const size_t es = bf ? 2 : 4, n = (size_t)rows * D, n_out = ((size_t)rows + 8) * D;
    DevScope dev(c);
    const void* dL = dev.upload((const char*)last_host, n * es);
    const void* dP = dev.upload((const char*)prev_host, n * es);
    void* dO = dev.filled(n_out * es, 0xFF);
    // the production form: the op and w in row 1 of a step table whose other rows hold 0xFF bytes, the step state at that row
    std::vector<AffineRow> tab(3);
    memset((void*)tab.data(), 0xFF, tab.size() * sizeof(AffineRow));
    tab[1].pad1 = op; tab[1].pad2 = __builtin_bit_cast(int, w);
    const StepState st_host{1, 0.f, 0ull, 1, 0};
    const AffineRow* dT = table ? dev.upload(tab.data(), tab.size() * sizeof(AffineRow)) : nullptr;
    const StepState* dS = table ? dev.upload(&st_host, sizeof(StepState)) : nullptr;
    auto once = [&]() { return launch_cache_extrapolate(dL, dP, dO, (long long)n, bf, dS, dT, table ? -1 : op, table ? __builtin_nanf("") : w, s); };
    DEV_HIP(dev, once());
    DEV_HIP(dev, hipStreamSynchronize(s));
    dev.download(out_host, dO, n_out * es);
    DEV_HIP(dev, time_launches(s, iters, once, ms_out));
    return dev.status();
}

int dd_dev_embed(dd_ctx* c, int B, int C, int S, int P, int D, int extras, int num_classes, int normalize, int generic, const float* x_img,
                 const float* w, const float* bias, const float* pos, const float* label_emb, const long long* y, const float* t_vec,
                 float t_state, const float* ln, float* x_tok_host, unsigned short* ln_frag_host, int iters, void* stream, float* ms_out) {
    if (!c || B < 1 || C < 1 || P < 1 || S < P || S % P || D < 2 || extras < 1 || extras > 2 || !x_img || !w || !bias || !pos || !x_tok_host ||
        (extras == 2 && (!label_emb || !y || num_classes < 1)) || (ln && !ln_frag_host) || iters < 0)
        return DD_ERR_INVALID;
    const int pd = C * P * P, L = extras + (S / P) * (S / P), Mp = round_up(B * L, 256);
    if (pd > 64) return ctx_fail(c, DD_ERR_UNSUPPORTED, "embed: patch_dim <= 64");
    hipStream_t s = (hipStream_t)stream;
    const std::vector<float> wt = transposed(w, D, pd);
    const size_t n_tok = ((size_t)Mp + 8) * D;
    EmbedArgs a{};
    a.B = B; a.C = C; a.S = S; a.P = P; a.D = D; a.L = L; a.extras = extras; a.num_classes = num_classes; a.normalize = normalize; a.Mp = Mp;
    a.generic = generic;
    if (ln && !embed_ln_supported(a)) return ctx_fail(c, DD_ERR_UNSUPPORTED, "embed with norm1: the MFMA kernel at patch 4, 3 channels, embed_dim 512");
    DevScope dev(c);
    a.x_img = dev.upload(x_img, (size_t)B * C * S * S * 4);
    a.wt = dev.upload(wt.data(), wt.size() * 4);
    a.bias = dev.upload(bias, (size_t)D * 4);
    a.pos = dev.upload(pos, (size_t)L * D * 4);
    if (extras == 2) { a.label_emb = dev.upload(label_emb, (size_t)num_classes * D * 4); a.y = dev.upload(y, (size_t)B * 8); }
    if (t_vec) a.t_vec = dev.upload(t_vec, (size_t)B * 4);
    a.st = dev.alloc<StepState>(sizeof(StepState));
    a.x_tok = dev.filled<float>(n_tok * 4, 0xFF);
    if (ln) {
        a.ln_g = dev.upload(ln, (size_t)2 * D * 4); a.ln_b = a.ln_g + D;
        a.ln_frag = dev.filled<bf16_t>(n_tok * 2, 0xFF);
    }
    DEV_HIP(dev, launch_set_state_float(a.st, t_state, s));      // t_vec NULL: the kernel's timestep; always: t, which it copies to t_final
    auto once = [&]() { return launch_embed(a, s); };
    DEV_HIP(dev, once());
    DEV_HIP(dev, hipStreamSynchronize(s));
    dev.download(x_tok_host, a.x_tok, n_tok * 4);
    if (ln) dev.download(ln_frag_host, a.ln_frag, n_tok * 2);
    DEV_HIP(dev, time_launches(s, iters, once, ms_out));
    return dev.status();
}

int dd_dev_time_mlp(dd_ctx* c, int B, int D, int L, int extras, int normalize, const float* w1, const float* b1, const float* w2,
                    const float* b2, const float* pos, const float* t_vec, float t_state, float* x_tok_host, int iters, void* stream,
                    float* ms_out) {
    if (!c || B < 1 || D < 2 || extras < 1 || L < extras || !w1 || !b1 || !w2 || !b2 || !pos || !x_tok_host || iters < 0) return DD_ERR_INVALID;
    if ((size_t)5 * D * 4 > 64 * 1024) return ctx_fail(c, DD_ERR_UNSUPPORTED, "time_mlp: 5 D floats of LDS");
    hipStream_t s = (hipStream_t)stream;
    const int H4 = 4 * D;
    const std::vector<float> w1t = transposed(w1, H4, D), w2t = transposed(w2, D, H4);
    const size_t n_tok = (size_t)B * L * D;
    DevScope dev(c);
    StepState* st = dev.alloc<StepState>(sizeof(StepState));
    float* dX = dev.upload(x_tok_host, n_tok * 4);
    const TimeMlpArgs a{dev.upload(w1t.data(), w1t.size() * 4), dev.upload(b1, (size_t)H4 * 4), dev.upload(w2t.data(), w2t.size() * 4),
                        dev.upload(b2, (size_t)D * 4), dev.upload(pos, (size_t)L * D * 4), t_vec ? dev.upload(t_vec, (size_t)B * 4) : nullptr,
                        st, dX, B, D, L, extras, normalize};
    DEV_HIP(dev, launch_set_state_float(st, t_state, s));
    auto once = [&]() { return launch_time_mlp(a, s); };
    DEV_HIP(dev, once());
    DEV_HIP(dev, hipStreamSynchronize(s));
    dev.download(x_tok_host, dX, n_tok * 4);
    DEV_HIP(dev, time_launches(s, iters, once, ms_out));
    return dev.status();
}

int dd_dev_vae_gather(dd_ctx* c, int kind, int precision, int B, int H, int W, int Cn, const void* src_host, void* dst_host, size_t dst_bytes,
                      void* stream) {
    const bool bf = precision == DD_PREC_BF16;
    if (!c || (!bf && precision != DD_PREC_FP32) || kind < 0 || kind > 3 || B < 1 || H < 1 || W < 1 || !src_host || !dst_host) return DD_ERR_INVALID;
    if (kind == 3 && (H % 2 || W % 2)) return DD_ERR_INVALID;            // the 2x upsample of a whole source pixel grid
    hipStream_t s = (hipStream_t)stream;
    const size_t esz = bf ? 2 : 4, kt = 128 / esz;
    const int C = kind == 1 ? 4 : Cn;
    if (C < 1) return DD_ERR_INVALID;
    const int Kpad = (int)((9 * (size_t)C + kt - 1) / kt * kt);          // as dd_vae_finalize pads a conv's K to the GEMM k-tile
    const size_t rows = (size_t)B * H * W, need = rows * Kpad * esz;
    if (dst_bytes < need) return ctx_fail(c, DD_ERR_INVALID, "vae_gather: dst_bytes below B H W Kpad elements");
    if (kind != 1 && C % (16 / (int)esz)) return ctx_fail(c, DD_ERR_UNSUPPORTED, "vae_gather: C must fill 16-byte vectors");
    DevScope dev(c);
    void* dD = dev.filled(dst_bytes, 0xFF);
    if (kind == 0) {
        const void* dS = dev.upload((const char*)src_host, rows * 4 * C * esz);
        DEV_HIP(dev, bf ? launch_im2col3x3_s2<bf16_t>((const bf16_t*)dS, (bf16_t*)dD, B, H, W, C, Kpad, s)
                        : launch_im2col3x3_s2<float>((const float*)dS, (float*)dD, B, H, W, C, Kpad, s));
    } else if (kind >= 2) {
        const int up = kind == 3;
        const void* dS = dev.upload((const char*)src_host, (up ? rows / 4 : rows) * C * esz);
        DEV_HIP(dev, bf ? launch_im2col3x3<bf16_t>((const bf16_t*)dS, (bf16_t*)dD, B, H, W, C, up, Kpad, s)
                        : launch_im2col3x3<float>((const float*)dS, (float*)dD, B, H, W, C, up, Kpad, s));
    } else {
        const float* dS = dev.upload((const float*)src_host, rows * 3 * 4);
        float* dI = dev.filled<float>(rows * 4 * 4, 0xFF);
        DEV_HIP(dev, launch_vae_image(dS, dI, B, H * W, s));
        DEV_HIP(dev, bf ? launch_im2col3x3_c4<bf16_t>(dI, (bf16_t*)dD, B, H, W, Kpad, s) : launch_im2col3x3_c4<float>(dI, (float*)dD, B, H, W, Kpad, s));
    }
    DEV_HIP(dev, hipStreamSynchronize(s));
    dev.download(dst_host, dD, dst_bytes);
    return dev.status();
}

// The KL-VAE kernels that are no gather (vae_kernels.hip), each alone: every output and scratch buffer has DD_DEV_VAE_TAIL elements behind the
// last one the launch may write, holds 0xFF bytes before the launch and is downloaded whole.
int dd_dev_groupnorm(dd_ctx* c, int precision, int B, int HW, int C, int swish, const float* x_host, const float* gamma, const float* beta,
                     void* out_host, float* part_host, void* stream) {
    const bool bf = precision == DD_PREC_BF16;
    if (!c || (!bf && precision != DD_PREC_FP32) || B < 1 || B > 4096 || HW < 1 || HW > (1 << 20) || C < 1 || C > (1 << 14) ||
        (long long)B * HW * C > (1ll << 28) || !x_host || !gamma || !beta || !out_host)
        return DD_ERR_INVALID;
    if (C % 128 || C > 1024) return ctx_fail(c, DD_ERR_UNSUPPORTED, "groupnorm: C % 128 == 0, C <= 1024");      // what launch_groupnorm refuses
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)B * HW * C, esz = bf ? 2 : 4;
    const size_t n_part = (size_t)groupnorm_partials(B, HW) + DD_DEV_VAE_TAIL;
    DevScope dev(c);
    const float* dX = dev.upload(x_host, n * 4);
    const float* dG = dev.upload(gamma, (size_t)C * 4);
    const float* dB = dev.upload(beta, (size_t)C * 4);
    float* dP = dev.filled<float>(n_part * 4, 0xFF);
    void* dO = dev.filled((n + DD_DEV_VAE_TAIL) * esz, 0xFF);
    DEV_HIP(dev, bf ? launch_groupnorm<bf16_t>(dX, dP, dG, dB, (bf16_t*)dO, B, HW, C, swish, s)
                    : launch_groupnorm<float>(dX, dP, dG, dB, (float*)dO, B, HW, C, swish, s));
    DEV_HIP(dev, hipStreamSynchronize(s));
    dev.download(out_host, dO, (n + DD_DEV_VAE_TAIL) * esz);
    if (part_host) dev.download(part_host, dP, n_part * 4);
    return dev.status();
}

int dd_dev_softmax_rows(dd_ctx* c, int precision, int rows, int n, float scale, const float* s_host, void* p_host, void* stream) {
    const bool bf = precision == DD_PREC_BF16;
    if (!c || (!bf && precision != DD_PREC_FP32) || rows < 1 || n < 1 || (long long)rows * n > (1ll << 28) || !s_host || !p_host) return DD_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const size_t cnt = (size_t)rows * n, esz = bf ? 2 : 4;
    DevScope dev(c);
    const float* dS = dev.upload(s_host, cnt * 4);
    void* dP = dev.filled((cnt + DD_DEV_VAE_TAIL) * esz, 0xFF);
    DEV_HIP(dev, bf ? launch_softmax_rows<bf16_t>(dS, (bf16_t*)dP, rows, n, scale, s) : launch_softmax_rows<float>(dS, (float*)dP, rows, n, scale, s));
    DEV_HIP(dev, hipStreamSynchronize(s));
    dev.download(p_host, dP, (cnt + DD_DEV_VAE_TAIL) * esz);
    return dev.status();
}

int dd_dev_vae_input(dd_ctx* c, int B, int HW, const float* z_host, const float* w, const float* b, float inv_scale, float* out_host,
                     void* stream) {
    if (!c || B < 1 || HW < 1 || (long long)B * HW > (1ll << 26) || !z_host || !w || !b || !out_host) return DD_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)B * HW * 4;
    DevScope dev(c);
    const float* dZ = dev.upload(z_host, n * 4);
    const float* dW = dev.upload(w, 16 * 4);
    const float* dB = dev.upload(b, 4 * 4);
    float* dO = dev.filled<float>((n + DD_DEV_VAE_TAIL) * 4, 0xFF);
    DEV_HIP(dev, launch_vae_input(dZ, dW, dB, inv_scale, dO, B, HW, s));
    DEV_HIP(dev, hipStreamSynchronize(s));
    dev.download(out_host, dO, (n + DD_DEV_VAE_TAIL) * 4);
    return dev.status();
}

int dd_dev_vae_output(dd_ctx* c, int B, int C, int HW, int ldc, const float* in_host, float* out_host, void* stream) {
    if (!c || B < 1 || HW < 1 || C < 1 || ldc < C || ldc > 4096 || (long long)B * HW > (1ll << 24) || !in_host || !out_host) return DD_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)B * C * HW;
    DevScope dev(c);
    const float* dI = dev.upload(in_host, (size_t)B * HW * ldc * 4);
    float* dO = dev.filled<float>((n + DD_DEV_VAE_TAIL) * 4, 0xFF);
    DEV_HIP(dev, launch_vae_output(dI, dO, B, C, HW, ldc, s));
    DEV_HIP(dev, hipStreamSynchronize(s));
    dev.download(out_host, dO, (n + DD_DEV_VAE_TAIL) * 4);
    return dev.status();
}

int dd_dev_vae_moments(dd_ctx* c, int B, int HW, const float* h_host, const float* w, const float* b, const float* eps_host,
                       float* moments_host, float* z_host, void* stream) {
    if (!c || B < 1 || HW < 1 || (long long)B * HW > (1ll << 26) || !h_host || !w || !b || (!moments_host && !z_host)) return DD_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const size_t px = (size_t)B * HW;
    DevScope dev(c);
    const float* dH = dev.upload(h_host, px * 8 * 4);
    const float* dW = dev.upload(w, 64 * 4);
    const float* dB = dev.upload(b, 8 * 4);
    const float* dE = eps_host ? dev.upload(eps_host, px * 4 * 4) : nullptr;
    float* dM = moments_host ? dev.filled<float>((px * 8 + DD_DEV_VAE_TAIL) * 4, 0xFF) : nullptr;
    float* dZ = z_host ? dev.filled<float>((px * 4 + DD_DEV_VAE_TAIL) * 4, 0xFF) : nullptr;
    DEV_HIP(dev, launch_vae_moments(dH, dW, dB, dE, dM, dZ, B, HW, s));
    DEV_HIP(dev, hipStreamSynchronize(s));
    if (moments_host) dev.download(moments_host, dM, (px * 8 + DD_DEV_VAE_TAIL) * 4);
    if (z_host) dev.download(z_host, dZ, (px * 4 + DD_DEV_VAE_TAIL) * 4);
    return dev.status();
}

int dd_dev_cast(dd_ctx* c, int precision, long long n, const float* x_host, void* out_host, void* stream) {
    const bool bf = precision == DD_PREC_BF16;
    if (!c || (!bf && precision != DD_PREC_FP32) || n < 1 || n > (1ll << 28) || !x_host || !out_host) return DD_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const size_t esz = bf ? 2 : 4;
    DevScope dev(c);
    const float* dX = dev.upload(x_host, (size_t)n * 4);
    void* dO = dev.filled(((size_t)n + DD_DEV_VAE_TAIL) * esz, 0xFF);
    DEV_HIP(dev, bf ? launch_cast<bf16_t>(dX, (bf16_t*)dO, n, s) : launch_cast<float>(dX, (float*)dO, n, s));
    DEV_HIP(dev, hipStreamSynchronize(s));
    dev.download(out_host, dO, ((size_t)n + DD_DEV_VAE_TAIL) * esz);
    return dev.status();
}

// The early-exit probes (rowops.hip), each through its production launch_* function on host arrays: every output has DD_DEV_EE_TAIL elements
// behind the last one the launch may write, holds 0xFF bytes before the launch and is downloaded whole.
int dd_dev_ee_probe(dd_ctx* c, int B, int L, int D, int n_probe, int t_state, int t_mul, int add, const float* x_host, const float* pw,
                    const float* pb, float* srow_host, float* out_host, void* stream) {
    if (!c || B < 1 || B > 4096 || L < 1 || D < 1 || (long long)B * L * D > (1ll << 28) || n_probe < 1 || n_probe > (1 << 20) || t_state < 0 ||
        t_state > 65535 || t_mul < 0 || t_mul > 65535 || add < 0 || !x_host || !pw || !pb || !srow_host)
        return DD_ERR_INVALID;
    const long long pi = (long long)t_state * t_mul + add;      // the probe row the launch reads
    if (pi >= n_probe) return DD_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const size_t rows = (size_t)B * L;
    DevScope dev(c);
    const float* dX = dev.upload(x_host, rows * D * 4);
    const float* dW = dev.upload(pw, (size_t)n_probe * D * 4);
    const float* dB = dev.upload(pb, (size_t)n_probe * 4);
    StepState* st = dev.alloc<StepState>(sizeof(StepState));
    float* dS = dev.filled<float>((rows + DD_DEV_EE_TAIL) * 4, 0xFF);
    float* dO = out_host ? dev.filled<float>(((size_t)B + DD_DEV_EE_TAIL) * 4, 0xFF) : nullptr;
    DEV_HIP(dev, launch_set_state(st, t_state, 0ull, s));
    DEV_HIP(dev, launch_ee_probe(dX, dW, dB, dO, dS, B, L, D, st, t_mul, add, s));
    DEV_HIP(dev, hipStreamSynchronize(s));
    dev.download(srow_host, dS, (rows + DD_DEV_EE_TAIL) * 4);
    if (out_host) dev.download(out_host, dO, ((size_t)B + DD_DEV_EE_TAIL) * 4);
    return dev.status();
}

int dd_dev_ee_probe_reduce(dd_ctx* c, int rows, int L, const float* srow_host, float* out_host, void* stream) {
    if (!c || rows < 1 || L < 1 || (long long)rows * L > (1ll << 28) || !srow_host || !out_host) return DD_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    DevScope dev(c);
    const float* dS = dev.upload(srow_host, (size_t)rows * L * 4);
    float* dO = dev.filled<float>(((size_t)rows + DD_DEV_EE_TAIL) * 4, 0xFF);
    DEV_HIP(dev, launch_ee_probe_reduce(dS, dO, rows, L, s));
    DEV_HIP(dev, hipStreamSynchronize(s));
    dev.download(out_host, dO, ((size_t)rows + DD_DEV_EE_TAIL) * 4);
    return dev.status();
}

int dd_dev_ee_attn_probe(dd_ctx* c, int B, int L, int D, const float* x_host, const float* q, const float* wkv, const float* bkv,
                         const float* w0, const float* b0, const float* w2, const float* b2, float* out_host, void* stream) {
    if (!c || B < 1 || B > 4096 || L < 2 || D < 64 || D % 64 || (long long)B * L * D > (1ll << 28) || !x_host || !q || !wkv || !bkv || !w0 || !b0 ||
        !w2 || !b2 || !out_host)
        return DD_ERR_INVALID;
    if (((size_t)L + 3 * (size_t)D) * 4 > 64 * 1024) return ctx_fail(c, DD_ERR_UNSUPPORTED, "ee_attn_probe: L + 3 D floats of LDS");
    hipStream_t s = (hipStream_t)stream;
    const AttnProbeFold f = fold_attn_probe(D, q, wkv, w0);      // as finalize folds the model's probes
    DevScope dev(c);
    const float* dX = dev.upload(x_host, (size_t)B * L * D * 4);
    const AttnProbeW w{dev.upload(f.u.data(), (size_t)D * 4), dev.upload(f.wvt.data(), (size_t)D * D * 4), dev.upload(bkv + D, (size_t)D * 4),
                       dev.upload(f.w0t.data(), (size_t)D * D * 4), dev.upload(b0, (size_t)D * 4), dev.upload(w2, (size_t)D * 4), dev.upload(b2, 4)};
    float* dO = dev.filled<float>(((size_t)B + DD_DEV_EE_TAIL) * 4, 0xFF);
    DEV_HIP(dev, launch_ee_attn_probe(dX, w, dO, B, L, D, s));
    DEV_HIP(dev, hipStreamSynchronize(s));
    dev.download(out_host, dO, ((size_t)B + DD_DEV_EE_TAIL) * 4);
    return dev.status();
}

}  // extern "C"

// dd_dev_final, and dd_dev_final_seeded with the n per-image seeds of the whole batch (seeds_host null: none)
static int dev_final(dd_ctx* c, dd_dev_final_args* p, const uint64_t* seeds_host, int n_seeds, void* stream) {
    if (!c || !p) return DD_ERR_INVALID;
    const dd_dev_final_args& q = *p;
    if (seeds_host && (q.b0 < 0 || q.B < 1 || n_seeds > (1 << 22) || (long long)n_seeds < (long long)q.b0 + q.B)) return DD_ERR_INVALID;
    // ---- everything the selected instantiation dereferences, before anything touches the GPU
    if (q.B < 1 || q.B > 4096 || q.C < 1 || q.C > 4 || q.P < 1 || q.P * q.P * q.C > 64 || q.S < q.P || q.S > 1024 || q.S % q.P || q.extras < 0 ||
        q.extras > 64 || q.b0 < 0 || q.images < q.B || q.images > 2 * q.B + 64 || !q.dec || !q.wconv || !q.bconv)
        return DD_ERR_INVALID;
    const int g = q.S / q.P, pd = q.P * q.P * q.C;
    if (q.L - q.extras != g * g || (long long)q.images * q.C * q.S * q.S > (1ll << 26)) return DD_ERR_INVALID;
    const bool cfg = q.pair_B > 0, ag = q.dec2 != nullptr, layered = q.layer_B > 0;
    if (q.pair_B < 0 || q.layer_B < 0 || (cfg && (q.pair_B != q.B || ag || q.images < 2 * q.pair_B))) return DD_ERR_INVALID;
    if (ag && (!q.wconv2 || !q.bconv2 || q.extras2 < 0 || q.extras2 > 64 || q.L2 - q.extras2 != g * g)) return DD_ERR_INVALID;
    if (layered && (cfg || ag || q.hist_row || q.known || q.B % q.layer_B || q.w_stride < 0 || q.b_stride < 0 || q.w_stride > (1 << 20) ||
                    q.b_stride > (1 << 20)))
        return DD_ERR_INVALID;
    if (q.noise_mode < DD_NOISE_NONE || q.noise_mode > DD_NOISE_PHILOX || (q.variance != DD_VAR_BETA_TILDE && q.variance != DD_VAR_BETA)) return DD_ERR_INVALID;
    if (q.t < 0 || q.t > (q.table ? 65535 : 999)) return DD_ERR_INVALID;
    if ((q.write_eps && !q.eps_out) || (q.write_x && (!q.x_in || !q.x_out)) || (q.write_x && q.noise_mode == DD_NOISE_BUFFER && !q.z)) return DD_ERR_INVALID;
    if (q.hist_row && (!q.table || !q.write_x || !q.h)) return DD_ERR_INVALID;
    if (q.known && (!q.write_x || !q.kx0 || !q.kmask)) return DD_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const size_t img = (size_t)q.C * q.S * q.S, n_in = (size_t)q.B * img, n_out = (size_t)q.images * img + 8;
    const int layers = layered ? q.B / q.layer_B : 1;
    const size_t t_rows = (size_t)q.t + 2;
    DevScope dev(c);
    FinalArgs fa{};
    // the head's arguments that the model and the chain determine (forward.hip final_args)
    fa.dec = dev.upload(q.dec, (size_t)(cfg ? 2 * q.pair_B : q.B) * q.L * pd * 4);
    fa.wconv = dev.upload(q.wconv, ((size_t)(layers - 1) * q.w_stride + (size_t)q.C * q.C * 9) * 4);
    fa.bconv = dev.upload(q.bconv, ((size_t)(layers - 1) * q.b_stride + q.C) * 4);
    fa.B = q.B; fa.C = q.C; fa.S = q.S; fa.P = q.P; fa.L = q.L; fa.extras = q.extras;
    // the step state and the context's coefficient table: row t alone holds the caller's coefficients
    const StepState st0{q.t, q.table ? q.row_t_model : (float)q.t, q.seed, q.t, 0};
    fa.st = dev.upload(&st0, sizeof st0);
    StepCoef* coef = dev.filled<StepCoef>(1000 * sizeof(StepCoef), 0xFF);
    if (!q.table && dev.ok()) {
        const StepCoef cf{q.c1, q.c2, q.sigma_tilde, q.sigma_beta};
        dev.ok(hipMemcpy(coef + q.t, &cf, sizeof cf, hipMemcpyHostToDevice), "hipMemcpy to the device");
    }
    fa.coef = coef;
    // the guidance of model_eps / run_guide, the batched early-exit heads of ee_finish
    if (cfg) { fa.pair_B = q.pair_B; fa.guide_scale = q.guide_scale; }
    if (ag) {
        fa.dec2 = dev.upload(q.dec2, (size_t)q.B * q.L2 * pd * 4);
        fa.wconv2 = dev.upload(q.wconv2, (size_t)q.C * q.C * 9 * 4); fa.bconv2 = dev.upload(q.bconv2, (size_t)q.C * 4);
        fa.L2 = q.L2; fa.extras2 = q.extras2; fa.guide_scale = q.guide_scale;
    }
    if (layered) { fa.layer_B = q.layer_B; fa.w_stride = q.w_stride; fa.b_stride = q.b_stride; }
    // what the launch writes (enqueue_step / forward_eps): canary bytes everywhere, or the caller's bytes (x aliased, h)
    float* dE = q.eps_out ? dev.filled<float>(n_out * 4, 0xFF) : nullptr;
    float* dX = nullptr;
    if (q.x_out) {
        dX = dev.filled<float>(n_out * 4, 0xFF);
        if (q.write_x && q.x_alias && dev.ok()) dev.ok(hipMemcpy(dX, q.x_in, (size_t)q.images * img * 4, hipMemcpyHostToDevice), "hipMemcpy to the device");
    }
    if (q.write_eps) fa.eps_out = dE;
    if (q.write_x) {
        fa.x_in = q.x_alias ? dX : dev.upload(q.x_in, (size_t)q.images * img * 4);
        fa.x_out = dX;
        if (q.noise_mode == DD_NOISE_BUFFER) fa.z = dev.upload(q.z, n_in * 4);
    }
    fa.noise_mode = q.noise_mode; fa.variance = q.variance; fa.advance = q.advance; fa.b0 = q.b0;
    if (q.table) {
        AffineRow* atab = dev.filled<AffineRow>(t_rows * sizeof(AffineRow), 0xFF);
        const AffineRow rows[2] = {{q.row_t_model, q.row_a, q.row_b, q.row_c, q.row_noise, q.row_ctr, 0, 0}, {q.next_t_model, 0.f, 0.f, 0.f, 0, 0, 0, 0}};
        if (dev.ok()) dev.ok(hipMemcpy(atab + q.t, rows, sizeof rows[0], hipMemcpyHostToDevice), "hipMemcpy to the device");
        if (dev.ok()) dev.ok(hipMemcpy(&atab[q.t + 1].t_model, &rows[1].t_model, sizeof(float), hipMemcpyHostToDevice), "hipMemcpy to the device");
        fa.atab = atab;
    }
    if (q.h) fa.h = dev.upload(q.h, n_out * 4);
    if (q.hist_row) {
        HistRow* htab = dev.filled<HistRow>(t_rows * sizeof(HistRow), 0xFF);
        const HistRow hr{q.hist_d, q.hist_p, q.hist_q, q.hist};
        if (dev.ok()) dev.ok(hipMemcpy(htab + q.t, &hr, sizeof hr, hipMemcpyHostToDevice), "hipMemcpy to the device");
        fa.htab = htab;
    }
    if (q.known) {
        KnownRow* ktab = dev.filled<KnownRow>((q.table ? t_rows : (size_t)1000) * sizeof(KnownRow), 0xFF);
        const KnownRow kr{q.known_ka, q.known_kb};
        if (dev.ok()) dev.ok(hipMemcpy(ktab + q.t, &kr, sizeof kr, hipMemcpyHostToDevice), "hipMemcpy to the device");
        fa.kx0 = dev.upload(q.kx0, n_in * 4); fa.kmask = dev.upload(q.kmask, (size_t)q.B * q.S * q.S * 4); fa.ktab = ktab;
    }
    if (seeds_host) fa.seeds = (const unsigned long long*)dev.upload(seeds_host, (size_t)n_seeds * sizeof(uint64_t));
    const hipError_t first = dev.ok() ? launch_final(fa, s) : hipSuccess;
    if (first == hipErrorInvalidValue) return ctx_fail(c, DD_ERR_INVALID, "final: a combination of operands launch_final refuses");      // (refused before any launch)
    DEV_HIP(dev, first);
    DEV_HIP(dev, hipStreamSynchronize(s));
    if (q.eps_out) dev.download(q.eps_out, dE, n_out * 4);
    if (q.x_out) dev.download(q.x_out, dX, n_out * 4);
    if (q.h) dev.download(q.h, fa.h, n_out * 4);
    StepState st1{};
    dev.download(&st1, fa.st, sizeof st1);
    if (dev.ok()) { p->t_out = st1.t; p->t_final_out = st1.t_final; p->t_model_out = st1.t_model; p->seed_out = st1.seed; }
    return dev.status();
}

// What the scan entries (dev_scan, dev_scan_exits) share.  The limits on the fields their two args structs have in common and on the seeds
// (own_ok: the entry's own limits), all DD_ERR_INVALID, then the shape the launchers refuse
template <typename Args>
static int scan_dev_check(dd_ctx* c, const Args& q, bool own_ok, const uint64_t* seeds_host, int n_seeds) {
    if (!own_ok || q.B < 1 || q.B > 4096 || q.C < 1 || q.S < 1 || q.S > 4096 || q.b0 < 0 || q.B_all > (1 << 20) || (long long)q.b0 + q.B > q.B_all ||
        q.k < 0 || q.k > 65535 || q.iters < 0 || q.iters > 10000 || (q.iters > 0 && q.advance))
        return DD_ERR_INVALID;
    if ((seeds_host != nullptr) != (n_seeds > 0) || n_seeds > (1 << 22) || (seeds_host && n_seeds < q.b0 + q.B)) return DD_ERR_INVALID;
    if (q.C > 4 || (long long)q.C * q.S * q.S > (1ll << 24)) return ctx_fail(c, DD_ERR_UNSUPPORTED, "scan: 1..4 channels, at most 2^24 elements per image");
    return DD_OK;
}
static const unsigned long long* scan_dev_seeds(DevScope& dev, const uint64_t* seeds_host, int n_seeds) {
    return seeds_host ? (const unsigned long long*)dev.upload(seeds_host, (size_t)n_seeds * sizeof(uint64_t)) : nullptr;
}
// an input between 8 + 8 elements the kernel must never read
static const float* scan_dev_fenced(DevScope& dev, const float* host, size_t elems) {
    float* d = dev.filled<float>((elems + 16) * 4, 0xFF);
    if (dev.ok()) dev.ok(hipMemcpy(d + 8, host, elems * 4, hipMemcpyHostToDevice), "hipMemcpy to the device");
    return d + 8;
}
// The launch and what follows it: launch(p->advance) once (refused by the launcher: DD_ERR_INVALID, nothing launched), results() downloads
// the entry's outputs, the step state is read back into the args, and iters > 0 times that many more launches
template <typename Args, typename Launch, typename Results>
static int scan_dev_run(dd_ctx* c, DevScope& dev, Args* p, const StepState* st, hipStream_t s, Launch&& launch, Results&& results) {
    const hipError_t first = dev.ok() ? launch(p->advance) : hipSuccess;
    if (first == hipErrorInvalidValue) return ctx_fail(c, DD_ERR_INVALID, "scan: operands the launcher refuses");      // (refused before any launch)
    DEV_HIP(dev, first);
    DEV_HIP(dev, hipStreamSynchronize(s));
    results();
    StepState st1{};
    dev.download(&st1, st, sizeof st1);
    if (dev.ok()) { p->t_out = st1.t; p->t_final_out = st1.t_final; p->t_model_out = st1.t_model; }
    if (p->iters > 0 && dev.ok()) {      // (advance == 0: the launch leaves the state as it found it)
        float ms = 0.f;
        DEV_HIP(dev, time_launches(s, p->iters, [&] { return launch(0); }, &ms));
        p->ms_out = ms;
    }
    return dev.status();
}

// dd_dev_scan_diffuse (m_host null, xt_host set) and dd_dev_scan_error (m_host and err_host set): the step state and the row table they share
static int dev_scan(dd_ctx* c, dd_dev_scan_args* p, const float* x0_host, const float* m_host, const uint64_t* seeds_host, int n_seeds,
                    float* xt_host, float* err_host, void* stream) {
    if (!c || !p || !x0_host || (!xt_host && (!m_host || !err_host))) return DD_ERR_INVALID;
    const dd_dev_scan_args& q = *p;
    if (int rc = scan_dev_check(c, q, ((long long)q.k + 1) * q.B_all <= (1ll << 24) && q.ctr >= 0, seeds_host, n_seeds)) return rc;
    if ((long long)q.B * q.C * q.S * q.S > (1ll << 26)) return DD_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)q.B * q.C * q.S * q.S, rows = (size_t)q.k + 2;
    DevScope dev(c);
    const StepState st0{q.k, q.t_model, q.seed, q.k, 0};
    StepState* st = dev.upload(&st0, sizeof st0);
    ScanRow* tab = dev.filled<ScanRow>(rows * sizeof(ScanRow), 0xFF);
    const ScanRow row{q.t_model, q.ka, q.kb, q.tz, q.t0, q.tx, q.ctr, 0};
    if (dev.ok()) dev.ok(hipMemcpy(tab + q.k, &row, sizeof row, hipMemcpyHostToDevice), "hipMemcpy to the device");
    if (dev.ok()) dev.ok(hipMemcpy(&tab[q.k + 1].t_model, &q.next_t_model, sizeof(float), hipMemcpyHostToDevice), "hipMemcpy to the device");
    const unsigned long long* seeds = scan_dev_seeds(dev, seeds_host, n_seeds);
    const float* dX0 = scan_dev_fenced(dev, x0_host, n);
    const float* dM = xt_host ? nullptr : scan_dev_fenced(dev, m_host, n);
    const size_t out_elems = xt_host ? n + 16 : ((size_t)q.k + 1) * q.B_all + 8;
    float* dOut = dev.filled<float>(out_elems * 4, 0xFF);
    return scan_dev_run(c, dev, p, st, s, [&](int advance) {
        return xt_host ? launch_scan_diffuse(dX0, dOut + 8, st, tab, seeds, q.B, q.C, q.S, q.b0, s)
                       : launch_scan_error(dX0, dM, dOut, st, tab, seeds, q.B, q.C, q.S, q.b0, q.B_all, advance, s);
    }, [&] { dev.download(xt_host ? xt_host : err_host, dOut, out_elems * 4); });
}

// dd_dev_scan_exits_error: scan_exits_error_kernel through launch_scan_exits_error, once.  The table has 1001 rows of 0xFF bytes; row t holds the
// caller's row, row `next` the next timestep's t_model, row 1000 the counter base ctr - k.
static int dev_scan_exits(dd_ctx* c, dd_dev_scan_exits_args* p, const float* x0_host, const float* outs_host, const float* eps_host,
                          const float* cls_host, const uint64_t* seeds_host, int n_seeds, float* mse_host, float* tgtu_host, float* pred_host,
                          void* stream) {
    if (!c || !p || !x0_host || !eps_host || !mse_host || !tgtu_host) return DD_ERR_INVALID;
    const dd_dev_scan_exits_args& q = *p;
    if (q.exits < 1 || (q.exits > 1 && (!outs_host || !cls_host || !pred_host))) return DD_ERR_INVALID;
    if (int rc = scan_dev_check(c, q, q.t >= 0 && q.t <= 999 && q.next >= 0 && q.next <= 999 && q.ctr >= q.k, seeds_host, n_seeds)) return rc;
    if (q.exits > 32) return ctx_fail(c, DD_ERR_UNSUPPORTED, "scan: at most 32 exits");
    if (((long long)q.k + 1) * q.exits * q.B_all > (1ll << 24) || (long long)q.B * q.C * q.S * q.S * q.exits > (1ll << 27)) return DD_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int E = q.exits;
    const size_t n = (size_t)q.B * q.C * q.S * q.S;
    DevScope dev(c);
    const StepState st0{q.t, q.t_model, q.seed, q.t, 0};
    StepState* st = dev.upload(&st0, sizeof st0);
    ScanRow* tab = dev.filled<ScanRow>((size_t)(SCAN_EXITS_ROWS + 1) * sizeof(ScanRow), 0xFF);
    const ScanRow row{q.t_model, q.ka, q.kb, q.tz, q.t0, q.tx, q.ctr, q.next}, base{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, q.ctr - q.k, 0};
    if (dev.ok() && q.next != q.t) dev.ok(hipMemcpy(&tab[q.next].t_model, &q.next_t_model, sizeof(float), hipMemcpyHostToDevice), "hipMemcpy to the device");
    if (dev.ok()) dev.ok(hipMemcpy(tab + q.t, &row, sizeof row, hipMemcpyHostToDevice), "hipMemcpy to the device");
    if (dev.ok()) dev.ok(hipMemcpy(tab + SCAN_EXITS_ROWS, &base, sizeof base, hipMemcpyHostToDevice), "hipMemcpy to the device");
    const unsigned long long* seeds = scan_dev_seeds(dev, seeds_host, n_seeds);
    const float* dX0 = scan_dev_fenced(dev, x0_host, n);
    const float* dEps = scan_dev_fenced(dev, eps_host, n);
    const float* dOuts = E > 1 ? scan_dev_fenced(dev, outs_host, n * (E - 1)) : nullptr;
    const float* dCls = E > 1 ? scan_dev_fenced(dev, cls_host, (size_t)(E - 1) * q.B) : nullptr;
    const size_t mse_elems = ((size_t)q.k + 1) * E * q.B_all + 8, pred_elems = ((size_t)q.k + 1) * (E - 1) * q.B_all + 8;
    float* dMse = dev.filled<float>(mse_elems * 4, 0xFF);
    float* dTgt = dev.filled<float>(mse_elems * 4, 0xFF);
    float* dPred = E > 1 ? dev.filled<float>(pred_elems * 4, 0xFF) : nullptr;
    return scan_dev_run(c, dev, p, st, s, [&](int advance) {
        return launch_scan_exits_error(dX0, dOuts, dEps, dCls, dMse, dTgt, dPred, st, tab, seeds, q.B, q.C, q.S, E, q.b0, q.B_all, advance, s);
    }, [&] {
        dev.download(mse_host, dMse, mse_elems * 4);
        dev.download(tgtu_host, dTgt, mse_elems * 4);
        if (E > 1) dev.download(pred_host, dPred, pred_elems * 4);
    });
}

extern "C" {

int dd_dev_scan_exits_error(dd_ctx* c, dd_dev_scan_exits_args* p, const float* x0_host, const float* outs_host, const float* eps_host,
                            const float* cls_host, const uint64_t* seeds_host, int n_seeds, float* mse_host, float* tgtu_host, float* pred_host,
                            void* stream) {
    return dev_scan_exits(c, p, x0_host, outs_host, eps_host, cls_host, seeds_host, n_seeds, mse_host, tgtu_host, pred_host, stream);
}

int dd_dev_scan_diffuse(dd_ctx* c, dd_dev_scan_args* p, const float* x0_host, const uint64_t* seeds_host, int n_seeds, float* xt_host, void* stream) {
    if (!xt_host) return DD_ERR_INVALID;
    return dev_scan(c, p, x0_host, nullptr, seeds_host, n_seeds, xt_host, nullptr, stream);
}
int dd_dev_scan_error(dd_ctx* c, dd_dev_scan_args* p, const float* x0_host, const float* m_host, const uint64_t* seeds_host, int n_seeds,
                      float* err_host, void* stream) {
    if (!m_host || !err_host) return DD_ERR_INVALID;
    return dev_scan(c, p, x0_host, m_host, seeds_host, n_seeds, nullptr, err_host, stream);
}

int dd_dev_final(dd_ctx* c, dd_dev_final_args* p, void* stream) { return dev_final(c, p, nullptr, 0, stream); }

int dd_dev_final_seeded(dd_ctx* c, dd_dev_final_args* p, const uint64_t* seeds_host, int n, void* stream) {
    if (!seeds_host || n < 1) return DD_ERR_INVALID;
    return dev_final(c, p, seeds_host, n, stream);
}

}  // extern "C"
