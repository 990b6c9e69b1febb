// The tail of a sampling step (gfx950): the output head (unpatchify + 3x3 conv) fused with the update, the unfused step kernels, the
// early-exit selection, the step-state setters and the image conversion.  The update itself is defined once, in step_update.h.
// All arithmetic here is fp32 in both precision modes.
#include "dd_internal.h"
#include "step_update.h"
#include "vec_access.h"

namespace dd {
namespace {

// ------------------------------------------------------------------------------------------
// Output head (after final LayerNorm + decoder_pred GEMM) + the step update: unpatchify ("B (h w) (p1 p2 C) -> B C (h p1) (w p2)",
// reference models/uvit.py:125-132), 3x3 conv pad 1 (:382), then the update of step_update.h on the pixel; eps never goes to HBM
// unless asked for.  A workgroup owns a 16x16 pixel tile of one image and first parks the 18x18xC halo of the unpatchified decoder
// output in LDS, so every decoder value is fetched once instead of up to nine times (a tap outside the image multiplies a zero of the
// halo: fmaf(w, 0, acc) == acc).  An image smaller than a tile (the test models' 8x8) is one tile with 64 live lanes.
// CT = the channel count at compile time (3, 4; 0: a.C at run time): with it the 9 C^2 conv weights are unconditional scalar loads, one
// output channel's 9 C at a time, PT = the patch size likewise (the halo gather divides by it) -- the run-time form tested co < C / ci < C around every one of 144 candidate loads (221 scalar branches,
// 151 s_load_dword, the weights' SGPRs spilled to VGPR lanes: ~3 900 instructions for a kernel every sampling step waits for).
// G (classifier-free guidance, FinalArgs::pair_B): the workgroup of image b parks TWO halos, the conditional decoder rows of image b and the
// unconditional ones of image b + pair_B (2 x 13.8 KB of LDS), gathered by one loop so that both sets of loads are in flight together -- the
// alternative, a second gather into the one halo behind the first conv, would put a second dependent global round trip on a kernel that is
// a chain of them; then eps = eps_c + s (eps_c - eps_u) feeds the update, and x' goes to images b and b + pair_B.
// The second halo is a source of its own (FinalArgs::dec2, L2, extras2, wconv2, bconv2): for classifier-free guidance launch_final points
// it at the twin rows of dec and at the same conv; for autoguidance (pair_B == 0) it is the GUIDE model's decoder buffer of the same chain
// -- its own token count and its own 3x3 conv, a different layer -- and eps = eps_main + s (eps_main - eps_guide); nothing is written twice.
// H (multistep loop, FinalArgs::htab): the table-driven update gains the history term of row t, and h' goes back to h (image b's slot:
// guided, the conditional image only); H = false compiles to the code without it.  The h pixels are requested with x_in, ahead of the halo
// gather and without waiting for row t's hist flag (a load behind the step state -> row chain would hold the gather back); a step without
// history loads them but never lets them into x', so a NaN in h (the first step, an uninitialised buffer) cannot reach the result.
// K (known region, FinalArgs::kx0): x' is finished by known() of step_update.h in front of the x_out store.  The x0 and mask pixels are requested with
// x_in for the same reason as h, row t of ktab rides behind the step state beside the rule's own row, and the second Philox draw (z2, its own
// stream word) is issued beside the first: nothing is added to the chain of dependent round trips.  Guided, the twin image gets x'' too.
// K = false compiles to the code without any of it.
// ------------------------------------------------------------------------------------------
template <int CT, int PT, bool G, bool H, bool K>
__global__ void __launch_bounds__(256) final_tiled_kernel(const FinalArgs a) {
#pragma clang fp contract(off)
    // (row pitch 48 = 16 mod 32 words: the two 16-pixel rows a 32-lane group reads fall into disjoint bank halves; pitch 19 gave every tap read
    // a 2-way conflict on three banks -- 1.7 conflict cycles per LDS-active cycle in the round 2-4 profiles, for a kernel that is latency, not LDS)
    constexpr int NH = G ? 2 : 1;     // halos: conditional (, unconditional)
    __shared__ float u[NH][4][18][48];
    const int S = a.S, P = PT ? PT : a.P, C = CT ? CT : a.C, g = S / P, pd = P * P * C;
    const int tiles = (S + 15) / 16;
    const int b = blockIdx.x / (tiles * tiles), ty = (blockIdx.x / tiles) % tiles, tx = blockIdx.x % tiles;
    const int tid = threadIdx.x;
    const int ly = tid >> 4, lx = tid & 15, y = ty * 16 + ly, x = tx * 16 + lx;
    const bool inside = y < S && x < S;
    // Everything that does not depend on the decoder output is requested / computed first, so that its latency (step
    // state -> coefficient row, the x_t pixels, the Philox normals) overlaps the halo gather instead of following it:
    // the kernel is a chain of dependent memory round trips, not bandwidth.
    const StepRule<H> rule(a.st, a.coef, a.atab, a.htab, a.noise_mode, a.variance, a.advance);
    float xin[4] = {0.f, 0.f, 0.f, 0.f}, zin[4] = {0.f, 0.f, 0.f, 0.f}, hin[4] = {0.f, 0.f, 0.f, 0.f};
    float kin[4] = {0.f, 0.f, 0.f, 0.f}, z2in[4] = {0.f, 0.f, 0.f, 0.f}, km = 0.f;
    const KnownRule krule(K ? a.ktab : nullptr, rule.table, rule.t, a.noise_mode);
    if (inside && a.x_out) {
        if constexpr (K) km = a.kmask[((long long)b * S + y) * S + x];
#pragma unroll
        for (int co = 0; co < 4; ++co) {
            if (co < C) {
                const long long e = (((long long)b * C + co) * S + y) * S + x;
                xin[co] = a.x_in[e];
                if (rule.reads_z()) zin[co] = a.z[e];
                if constexpr (H) hin[co] = a.h[e];     // (not behind the row: used only where hr.hist is set)
                if constexpr (K) kin[co] = a.kx0[e];
            }
        }
    }
    const int layer = a.layer_B > 0 ? b / a.layer_B : 0;      // (early-exit heads batched into one launch: this image's layer)
    const float* wconv = a.wconv + layer * a.w_stride;
    const float* bconv = a.bconv + layer * a.b_stride;
    for (int idx = tid; idx < NH * 18 * 18; idx += 256) {
        const int hh = NH == 1 ? 0 : idx / (18 * 18), hi = NH == 1 ? idx : idx - hh * (18 * 18);
        const int hy = hi / 18, hx = hi % 18;
        const int yy = ty * 16 + hy - 1, xx = tx * 16 + hx - 1;
        const bool in = yy >= 0 && yy < S && xx >= 0 && xx < S;
        const bool second = NH == 2 && hh == 1;   // the second halo's own source
        const float* src = (second ? a.dec2 : a.dec) + ((long long)b * (second ? a.L2 : a.L) + (second ? a.extras2 : a.extras) + (in ? (yy / P) * g + (xx / P) : 0)) * pd +
                           (in ? ((yy % P) * P + (xx % P)) * C : 0);
        for (int ci = 0; ci < C; ++ci) u[hh][ci][hy][hx] = in ? src[ci] : 0.f;
    }
    if (inside && a.x_out && rule.draws()) {   // (key, id) of the pixel within the WHOLE batch (b0: this launch's first image), or under the image's own seed: draw_site
        const DrawSite ds = draw_site(a.seeds, a.st->seed, (unsigned long long)(b + a.b0), (unsigned long long)(y * S + x), (unsigned long long)S * S);
        const f32x4 zn = philox_normal4(ds.key, ds.id, rule.ctr);
#pragma unroll
        for (int co = 0; co < 4; ++co) zin[co] = zn[co];
    }
    if constexpr (K) {
        if (inside && a.x_out && krule.draws()) {   // z2: the same key, pixel id and counter as z, the known region's stream word
            const DrawSite ds = draw_site(a.seeds, a.st->seed, (unsigned long long)(b + a.b0), (unsigned long long)(y * S + x), (unsigned long long)S * S);
            const f32x4 zn = philox_normal4(ds.key, ds.id, rule.ctr, PHILOX_KNOWN);
#pragma unroll
            for (int co = 0; co < 4; ++co) z2in[co] = zn[co];
        }
    }
    __syncthreads();
    if (blockIdx.x == 0 && tid == 0) rule.advance(a.st);
    if (!inside) return;
    constexpr int CM = CT ? CT : 4;
    float acc[NH][4] = {};
#pragma unroll
    for (int hh = 0; hh < NH; ++hh) {
        float uu[CM][9];
#pragma unroll
        for (int ci = 0; ci < CM; ++ci)
#pragma unroll
            for (int k = 0; k < 9; ++k) uu[ci][k] = ci < C ? u[hh][ci][ly + k / 3][lx + k % 3] : 0.f;
#pragma unroll
        for (int co = 0; co < CM; ++co) {
            if (co < C) {
                // uniform address, constant address space: scalar loads (s_load_dwordx8 ...), one output channel's 9 C weights live at a time
                const __attribute__((address_space(4))) float* wp = (const __attribute__((address_space(4))) float*)((G && hh == 1 ? a.wconv2 : wconv) + co * C * 9);
                float v = (G && hh == 1 ? a.bconv2 : bconv)[co];
#pragma unroll
                for (int k = 0; k < 9; ++k)
#pragma unroll
                    for (int ci = 0; ci < CM; ++ci)
                        if (ci < C) v = fmaf(wp[ci * 9 + k], uu[ci][k], v);
                acc[hh][co] = v;
            }
        }
    }
    if constexpr (G) {
#pragma unroll
        for (int co = 0; co < 4; ++co) {
            const float d = acc[0][co] - acc[1][co];
            acc[0][co] = acc[0][co] + a.guide_scale * d;
        }
    }
    const long long pair = G ? (long long)a.pair_B * C * S * S : 0;   // element offset of the unconditional twin of image b
#pragma unroll
    for (int co = 0; co < 4; ++co) {
        if (co < C) {
            const long long e = (((long long)b * C + co) * S + y) * S + x;
            const float eps = acc[0][co];
            if (a.eps_out) a.eps_out[e] = eps;
            if (a.x_out) {
                float v = rule.apply(xin[co], eps, zin[co], hin[co]);
                if constexpr (H) a.h[e] = rule.history(xin[co], eps);
                if constexpr (K) v = krule.apply(v, kin[co], km, z2in[co]);
                a.x_out[e] = v;
                if (G && a.pair_B > 0) a.x_out[e + pair] = v;     // (the twin exists under classifier-free guidance only)
            }
        }
    }
}

// the unfused known-region rule on [B, C, S, S] (dd_known_blend): the mask is shared by a pixel's channels; x and out may alias
__global__ void known_blend_kernel(const float* x, const float* __restrict__ x0, const float* __restrict__ mask, const float* __restrict__ z2,
                                   float* out, float ka, float kb, long long chw, long long hw, long long n) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool use_z2 = z2 != nullptr && kb != 0.f;
    out[i] = known(x[i], x0[i], mask[(i / chw) * hw + i % hw], ka, kb, use_z2 ? z2[i] : 0.f, use_z2);
}

// the unfused update on n elements from coefficients passed by value (dd_ddpm_step / dd_ddpm_step_coef)
__global__ void ddpm_step_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                 const float* __restrict__ z, float* __restrict__ out, StepCoef c,
                                 int use_noise, int variance_beta, long long n) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const StepRule<false> rule(c, variance_beta != 0, use_noise != 0);
    out[i] = rule.apply(x[i], eps[i], rule.reads_z() ? z[i] : 0.f, 0.f);
}

// Exit selection and the update in one launch (the device-resident early-exit loop: two launches less on every step's serial tail,
// and the selected model output never travels through HBM): per pixel, the image's exit layer from cls, then the update on
// (outputs ++ [eps])[idx], z from the Philox generator of the fused step (same counter: pixel, t).  x [B, C, S, S] in place; b0: a
// half-batch chain's first image within the whole batch; seeds: the whole batch's per-image seeds or null (draw_site).
__global__ void __launch_bounds__(256) ee_select_step_kernel(float* __restrict__ x, const float* __restrict__ outs, const float* __restrict__ eps,
                                                             const float* __restrict__ cls, float thr, int depth, int* __restrict__ idx_out,
                                                             int idx_stride, int idx_col0, StepState* st, const StepCoef* __restrict__ coef,
                                                             int B, int C, int S, int noise_mode, int advance, int b0,
                                                             const unsigned long long* __restrict__ seeds) {
#pragma clang fp contract(off)
    const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long hw = (long long)S * S;
    const StepRule<false> rule(st, coef, nullptr, nullptr, noise_mode == 2 ? 2 : 0, 0, advance);   // (this loop draws on the device or not at all)
    if (pix == 0) rule.advance(st);
    if (pix >= (long long)B * hw) return;
    const long long b = pix / hw, p = pix - b * hw;
    f32x4 zn = {0.f, 0.f, 0.f, 0.f};
    if (rule.draws()) {
        const DrawSite ds = draw_site(seeds, st->seed, (unsigned long long)(b + b0), (unsigned long long)p, (unsigned long long)hw);
        zn = philox_normal4(ds.key, ds.id, rule.ctr);
    }
    const int idx = ee_exit_layer(cls, thr, depth, B, (int)b);
    if (idx_out && p == 0) idx_out[(long long)rule.t * idx_stride + idx_col0 + b] = idx;     // row t of indices_by_timestep (eesampler.py:71)
    const float* src = idx == depth ? eps : outs + (long long)idx * B * C * hw;
    for (int c = 0; c < C; ++c) {
        const long long e = (b * C + c) * hw + p;
        x[e] = rule.apply(x[e], src[e], zn[c], 0.f);
    }
}

// out = a*x + b*m + c*z, each product rounded (no FMA contraction): the common form of the reference's
// predict_original / predict_previous post-processing (sampler.py:59-79) and of a DDIM step (:112-120).
__global__ void affine_step_kernel(const float* __restrict__ x, const float* __restrict__ m,
                                   const float* __restrict__ z, float* __restrict__ out, float a, float b, float c,
                                   long long n) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const StepRule<false> rule(a, b, c, HistRow{0.f, 0.f, 0.f, 0}, z != nullptr);
    out[i] = rule.apply(x[i], m[i], rule.reads_z() ? z[i] : 0.f, 0.f);
}

// out = a*x + b*m [+ d*h if use_hist] [+ c*z if z], then h = p*x + q*m: the multistep row (dd_multistep_step, DPM-Solver++), the update the
// multistep output head fuses.  h is not read when use_hist is 0; x and out may alias (in place), h must alias neither.
__global__ void multistep_step_kernel(const float* x, const float* __restrict__ m, const float* __restrict__ z, float* h, float* out,
                                      float a, float b, float c, float d, float p, float q, int use_hist, long long n) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const StepRule<true> rule(a, b, c, HistRow{d, p, q, use_hist}, z != nullptr);
    const float xv = x[i], mv = m[i];
    const float v = rule.apply(xv, mv, rule.reads_z() ? z[i] : 0.f, rule.hr.hist ? h[i] : 0.f);
    h[i] = rule.history(xv, mv);
    out[i] = v;
}

// ------------------------------------------------------------------------------------------
// The thresholded multistep step (step_update.h: x0 thresholding; ThresholdArgs), one workgroup of 1024 threads per image.  It needs an
// order statistic of the image's |x0| inside the step, so it cannot ride in the output head: that launch writes the (guided) m of the step
// and this one finishes it.  Like the head it is a chain of dependent round trips, so every global load is issued up front -- x, m, h, and
// where used z, the known image and the mask, W = 4 elements (16 bytes) per access -- and the Philox draws and the known region's
// ka x0 + kb z2 are computed in their shadow; a thread keeps its 16 elements' operands in registers across the selection.
//   1. x0 = p x + q m goes to LDS (at most 16 384 floats, 64 KB).
//   2. dynamic: v[i] by a radix select on the keys bits(|x0|), which order as unsigned integers: four passes of 8-bit digits from the top,
//      each a 256-bin LDS histogram (integer LDS adds) of the keys that match the digits chosen so far, scanned by the first wave for the
//      bin that holds rank i.  One more pass counts the keys <= v[i] and takes the smallest key above: v[i + 1] is that key if exactly
//      i + 1 keys are <= v[i] (and i + 1 < n), else v[i].  Exact, deterministic (integer adds commute), five passes for any bits.
//   3. s, xh = clamp(x0, +-s) / s (static: clamp alone), the update, the known region, the stores: x' (guided: the twin image too), h' = xh.
// x and out may alias: a thread reads its own elements before it writes them, and no workgroup reads another image (the twin is only written).
// W = 1: the same with scalar accesses (S * S no multiple of 4, or a pointer not 16-byte aligned).
// ------------------------------------------------------------------------------------------
template <int W>
__global__ void __launch_bounds__(1024) threshold_step_kernel(const ThresholdArgs a) {
#pragma clang fp contract(off)
    constexpr int NT = 1024, SLOTS = THRESHOLD_MAX_ELEMS / NT / W;     // a thread's share: 16 elements, in SLOTS accesses
    __shared__ __attribute__((aligned(16))) float x0s[THRESHOLD_MAX_ELEMS];
    __shared__ unsigned hist[256];
    __shared__ unsigned sel[4];      // the pass's digit, the rank within it; keys <= v[i], the smallest key above v[i]
    const int tid = threadIdx.x, b = blockIdx.x;
    const int hw = a.S * a.S, n = a.C * hw;
    const long long base = (long long)b * n;
    const bool loop = a.st != nullptr;
    const StepRule<true> rule = loop ? StepRule<true>(a.st, a.coef, a.atab, a.htab, a.noise_mode, 0, a.advance)
                                     : StepRule<true>(a.row.a, a.row.b, a.row.c, a.hr, a.z != nullptr);
    const bool kn_on = a.kx0 != nullptr;
    const KnownRule krule(kn_on ? a.ktab : nullptr, true, rule.t, a.noise_mode);
    float xv[SLOTS][W], hv[SLOTS][W], zv[SLOTS][W], kv[SLOTS][W], km[SLOTS][W];
    // ---- 1. every load, x0 to LDS
#pragma unroll
    for (int j = 0; j < SLOTS; ++j) {
        const int e0 = (tid + j * NT) * W;
#pragma unroll
        for (int w = 0; w < W; ++w) { xv[j][w] = 0.f; hv[j][w] = 0.f; zv[j][w] = 0.f; kv[j][w] = 0.f; km[j][w] = 0.f; }
        if (e0 < n) {
            float mv[W];
            load_w<W>(xv[j], a.x + base + e0);
            load_w<W>(mv, a.m + base + e0);
            load_w<W>(hv[j], a.h + base + e0);            // (not behind the row: used only where hr.hist is set)
            if (rule.reads_z()) load_w<W>(zv[j], a.z + base + e0);
            if (kn_on) {
                load_w<W>(kv[j], a.kx0 + base + e0);
                load_w<W>(km[j], a.kmask + (long long)b * hw + e0 % hw);
            }
            float x0[W];
#pragma unroll
            for (int w = 0; w < W; ++w) x0[w] = rule.history(xv[j][w], mv[w]);
            store_w<W>(&x0s[e0], x0);
        }
    }
    // Philox z (and the known region's z2): the (key, id) of draw_site, the step's counter, the two stream words, as final_tiled_kernel draws
    // them -- one draw serves a pixel's channels, so a slot reuses the previous slot's draws where it holds the same pixels of the next channel
    const bool zdraw = rule.draws(), z2draw = kn_on && krule.draws();
    if (zdraw || z2draw) {
        const unsigned long long seed = a.st->seed;
        f32x4 zc[W], z2c[W];
        int drawn = -1;
#pragma unroll
        for (int j = 0; j < SLOTS; ++j) {
            const int e0 = (tid + j * NT) * W;
            if (e0 < n) {
                const int c = e0 / hw, pix = e0 - c * hw;
                if (pix != drawn) {
#pragma unroll
                    for (int w = 0; w < W; ++w) {
                        const DrawSite ds = draw_site(a.seeds, seed, (unsigned long long)(b + a.b0), (unsigned long long)(pix + w), (unsigned long long)hw);
                        if (zdraw) zc[w] = philox_normal4(ds.key, ds.id, rule.ctr);
                        if (z2draw) z2c[w] = philox_normal4(ds.key, ds.id, rule.ctr, PHILOX_KNOWN);
                    }
                    drawn = pix;
                }
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    if (zdraw) zv[j][w] = pick(zc[w], c);
                    if (kn_on) kv[j][w] = krule.value(kv[j][w], z2draw ? pick(z2c[w], c) : 0.f);
                }
            }
        }
    } else if (kn_on) {
#pragma unroll
        for (int j = 0; j < SLOTS; ++j)
#pragma unroll
            for (int w = 0; w < W; ++w) kv[j][w] = krule.value(kv[j][w], 0.f);
    }
    __syncthreads();
    if (b == 0 && tid == 0) rule.advance(a.st);      // (no workgroup reads t / t_model)
    // ---- 2. the image's scale
    float s = a.thr.range;
    if (a.thr.dynamic) {
        unsigned prefix = 0, pmask = 0, rank = (unsigned)a.thr.i;
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
#pragma unroll
            for (int j = 0; j < SLOTS; ++j) {
                const int e0 = (tid + j * NT) * W;
                if (e0 < n) {
                    float v[W];
                    load_w<W>(v, &x0s[e0]);
#pragma unroll
                    for (int w = 0; w < W; ++w) {
                        const unsigned key = __float_as_uint(v[w]) & 0x7fffffffu;
                        if ((key & pmask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
                    }
                }
            }
            __syncthreads();
            if (tid < 64) {      // bins 4 tid .. 4 tid + 3; the lane whose bins hold the rank names the digit
                const unsigned c0 = hist[4 * tid], c1 = hist[4 * tid + 1], c2 = hist[4 * tid + 2], c3 = hist[4 * tid + 3];
                const unsigned sum = c0 + c1 + c2 + c3;
                unsigned inc = sum;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const unsigned up = __shfl_up(inc, o);
                    if (tid >= o) inc += up;
                }
                const unsigned exc = inc - sum;
                if (rank >= exc && rank < inc) {
                    unsigned r = rank - exc, dg = 0;
                    if (r >= c0) { r -= c0; dg = 1; if (r >= c1) { r -= c1; dg = 2; if (r >= c2) { r -= c2; dg = 3; } } }
                    sel[0] = 4 * tid + dg; sel[1] = r;
                }
            }
            __syncthreads();
            prefix |= sel[0] << shift; pmask |= 0xffu << shift; rank = sel[1];
        }
        if (tid == 0) { sel[2] = 0; sel[3] = 0xffffffffu; }
        __syncthreads();
        unsigned le = 0, above = 0xffffffffu;
#pragma unroll
        for (int j = 0; j < SLOTS; ++j) {
            const int e0 = (tid + j * NT) * W;
            if (e0 < n) {
                float v[W];
                load_w<W>(v, &x0s[e0]);
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    const unsigned key = __float_as_uint(v[w]) & 0x7fffffffu;
                    if (key <= prefix) ++le;
                    else above = min(above, key);
                }
            }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            le += __shfl_xor(le, o);
            above = min(above, (unsigned)__shfl_xor(above, o));
        }
        if ((tid & 63) == 0) { atomicAdd(&sel[2], le); atomicMin(&sel[3], above); }
        __syncthreads();
        const bool next = sel[2] == (unsigned)a.thr.i + 1u && a.thr.i + 1 < n;
        s = threshold_scale(__uint_as_float(prefix), __uint_as_float(next ? sel[3] : prefix), a.thr.f, a.thr.s_max);
    }
    // ---- 3. xh, the update, the known region, the stores
    const long long pair = (long long)a.pair_B * n;
#pragma unroll
    for (int j = 0; j < SLOTS; ++j) {
        const int e0 = (tid + j * NT) * W;
        if (e0 < n) {
            float x0[W], xh[W], out[W];
            load_w<W>(x0, &x0s[e0]);
#pragma unroll
            for (int w = 0; w < W; ++w) {
                xh[w] = threshold_clip(x0[w], s, a.thr.dynamic != 0);
                out[w] = rule.apply(xv[j][w], xh[w], zv[j][w], hv[j][w]);
                if (kn_on) out[w] = known_mix(out[w], kv[j][w], km[j][w]);
            }
            store_w<W>(a.h + base + e0, xh);
            store_w<W>(a.out + base + e0, out);
            if (a.pair_B > 0) store_w<W>(a.out + base + pair + e0, out);
        }
    }
}

// x_T on the device (dd_noise_images): out [B, C, S, S], channel c of pixel p of image b = component c of philox_normal4 at draw_site's (key, id)
// (b0 = 0), counter ctr, the stream word PHILOX_START -- independent of every step's z and z2 under the same key.  One draw serves a pixel's
// channels.  A thread owns W consecutive pixels of one image: W = 4 where hw % 4 == 0 and out is 16-byte aligned (one 16-byte store per
// channel), else W = 1 with plain stores.
template <int W>
__global__ void __launch_bounds__(256) noise_images_kernel(float* __restrict__ out, const unsigned long long* __restrict__ seeds, unsigned long long seed,
                                                           int ctr, int B, int C, int hw) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int per_image = hw / W;
    if (i >= (long long)B * per_image) return;
    const long long b = i / per_image;
    const int p0 = (int)(i - b * per_image) * W;
    f32x4 zn[W];
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const DrawSite ds = draw_site(seeds, seed, (unsigned long long)b, (unsigned long long)(p0 + w), (unsigned long long)hw);
        zn[w] = philox_normal4(ds.key, ds.id, ctr, PHILOX_START);
    }
    for (int c = 0; c < C; ++c) {
        float v[W];
#pragma unroll
        for (int w = 0; w < W; ++w) v[w] = pick(zn[w], c);
        store_w<W>(out + (b * C + c) * hw + p0, v);
    }
}

__global__ void set_state_kernel(StepState* st, int t, unsigned long long seed) {
    st->t = t;
    st->t_final = t;
    st->t_model = (float)t;
    st->seed = seed;
}
__global__ void set_state_table_kernel(StepState* st, const AffineRow* atab, unsigned long long seed) {
    st->t = 0;
    st->t_final = 0;
    st->t_model = atab[0].t_model;
    st->seed = seed;
}
// the label rows of one guided chain: [y [0, B) | null_label x B]
__global__ void __launch_bounds__(256) guided_labels_kernel(const long long* __restrict__ y, long long* __restrict__ out, int B, long long null_label) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < 2 * B) out[i] = i < B ? y[i] : null_label;
}
__global__ void set_state_float_kernel(StepState* st, float t) {
    st->t = (int)t;
    st->t_final = (int)t;
    st->t_model = t;
}

// reference sampler.py:145-146: samples = rearrange((x + 1) / 2, "b c h w -> b h w c").  One thread per pixel: the NCHW
// reads are coalesced per channel plane, the NHWC writes are C contiguous floats per thread.
__global__ void __launch_bounds__(256) to_images_kernel(const float* __restrict__ x, float* __restrict__ out, int B, int C, int S) {
    const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long hw = (long long)S * S;
    if (pix >= (long long)B * hw) return;
    const long long b = pix / hw, p = pix - b * hw;
    for (int c = 0; c < C; ++c) out[pix * C + c] = (x[(b * C + c) * hw + p] + 1.0f) / 2.0f;
}

// dd_early_exit_select: model_output[b] = (outputs ++ [eps])[idx[b]][b] with idx[b] = the image's exit layer (ee_exit_layer)
__global__ void ee_select_kernel(const float* __restrict__ outs, const float* __restrict__ eps, const float* __restrict__ cls,
                                 float thr, int depth, int B, long long chw, float* __restrict__ mo, int* __restrict__ idx_out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)B * chw) return;
    const int b = (int)(i / chw);
    const int idx = ee_exit_layer(cls, thr, depth, B, b);
    mo[i] = idx == depth ? eps[i] : outs[(long long)idx * B * chw + i];
    if (idx_out && i == (long long)b * chw) idx_out[b] = idx;
}

// eesampler.py:70: per-layer mean over the batch of the predicted errors (logging)
// (scale = 1 / B: the mean; scale = 1: the plain sum -- a half-batch chain's share, ee_mean_combine_kernel divides)
__global__ void __launch_bounds__(64) ee_batch_mean_kernel(const float* __restrict__ cls, float* __restrict__ err, int B,
                                                           const StepState* __restrict__ st, float scale) {
    const int k = blockIdx.x, lane = threadIdx.x;
    if (st) err += (long long)st->t_final * gridDim.x;            // row t of error_prediction_by_timestep (eesampler.py:70)
    float a = 0.f;
    for (int b = lane; b < B; b += 64) a += cls[(long long)k * B + b];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o);
    if (lane == 0) err[k] = scale == 1.0f ? a : a / (float)B;
}

// rows [t_lo, t_hi] of error_prediction_by_timestep from the two chains' per-step sums, in a fixed order: (chain 0 + chain 1) / B
__global__ void ee_mean_combine_kernel(const float* __restrict__ s0, const float* __restrict__ s1, float* __restrict__ err, int depth, int t_lo, int t_hi, int B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, n = (t_hi - t_lo + 1) * depth;
    if (i >= n) return;
    const long long e = (long long)t_lo * depth + i;
    err[e] = (s0[e] + s1[e]) / (float)B;
}

}  // namespace

// one instantiation per (C, P) specialisation x guidance x history x known region: (3, 4) CelebA-64 / ImageNet-64, (3, 2) CIFAR-10, (4, 2) 32 x 32 x 4
// latents (ImageNet-256), anything else the run-time form
template <int CT, int PT>
static void launch_final_cp(const FinalArgs& a, hipStream_t s) {
    const int tiles = (a.S + 15) / 16;
    const dim3 grid(a.B * tiles * tiles);       // guided (dec2 set): a.B images, each with a second decoder image
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, a); };
    if (a.kx0) {
        if (a.dec2) a.htab ? go(final_tiled_kernel<CT, PT, true, true, true>) : go(final_tiled_kernel<CT, PT, true, false, true>);
        else a.htab ? go(final_tiled_kernel<CT, PT, false, true, true>) : go(final_tiled_kernel<CT, PT, false, false, true>);
        return;
    }
    if (a.dec2) a.htab ? go(final_tiled_kernel<CT, PT, true, true, false>) : go(final_tiled_kernel<CT, PT, true, false, false>);
    else a.htab ? go(final_tiled_kernel<CT, PT, false, true, false>) : go(final_tiled_kernel<CT, PT, false, false, false>);
}

hipError_t launch_final(const FinalArgs& args, hipStream_t s) {
    FinalArgs a = args;
    if (a.pair_B > 0) {   // classifier-free guidance: the second halo is image b + pair_B of the same decoder buffer, under the same conv
        if (a.pair_B != a.B || a.layer_B > 0 || a.dec2) return hipErrorInvalidValue;
        a.dec2 = a.dec + (long long)a.pair_B * a.L * a.P * a.P * a.C;
        a.wconv2 = a.wconv; a.bconv2 = a.bconv; a.L2 = a.L; a.extras2 = a.extras;
    } else if (a.dec2 && (a.layer_B > 0 || !a.wconv2 || !a.bconv2 || a.L2 - a.extras2 != a.L - a.extras)) {   // autoguidance: same patch grid
        return hipErrorInvalidValue;
    }
    // the multistep loop: a table-driven step that writes x and h
    if (a.htab && (!a.atab || !a.h || !a.x_in || !a.x_out || a.layer_B > 0)) return hipErrorInvalidValue;
    // a known region finishes a step's x'
    if (a.kx0 && (!a.kmask || !a.ktab || !a.x_in || !a.x_out || a.layer_B > 0)) return hipErrorInvalidValue;
    if (a.C == 3 && a.P == 4) launch_final_cp<3, 4>(a, s);
    else if (a.C == 3 && a.P == 2) launch_final_cp<3, 2>(a, s);
    else if (a.C == 4 && a.P == 2) launch_final_cp<4, 2>(a, s);
    else launch_final_cp<0, 0>(a, s);
    return hipGetLastError();
}

hipError_t launch_ddpm_step(const float* x, const float* eps, const float* z, float* out, StepCoef c,
                            int use_noise, long long n, hipStream_t s) {
    // variance selection is folded by the caller into c.sigma_tilde
    hipLaunchKernelGGL(ddpm_step_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, eps, z, out, c,
                       use_noise, 0, n);
    return hipGetLastError();
}

hipError_t launch_known_blend(const float* x, const float* x0, const float* mask, const float* z2, float ka, float kb, float* out, int B, int C,
                              int S, hipStream_t s) {
    const long long hw = (long long)S * S, chw = hw * C, n = chw * B;
    hipLaunchKernelGGL(known_blend_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, x0, mask, z2, out, ka, kb, chw, hw, n);
    return hipGetLastError();
}

hipError_t launch_affine_step(const float* x, const float* m, const float* z, float* out, float a, float b, float c,
                              long long n, hipStream_t s) {
    hipLaunchKernelGGL(affine_step_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, m, z, out, a, b, c, n);
    return hipGetLastError();
}

hipError_t launch_multistep_step(const float* x, const float* m, const float* z, float* h, float* out, float a, float b, float c, float d,
                                 float p, float q, int use_hist, long long n, hipStream_t s) {
    hipLaunchKernelGGL(multistep_step_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, m, z, h, out, a, b, c, d, p, q, use_hist, n);
    return hipGetLastError();
}
hipError_t launch_threshold_step(const ThresholdArgs& a, hipStream_t s) {
    const long long hw = (long long)a.S * a.S, n = hw * a.C;
    if (a.B < 1 || n < 1 || n > THRESHOLD_MAX_ELEMS || !a.x || !a.m || !a.h || !a.out) return hipErrorInvalidValue;
    if (a.thr.dynamic && (a.thr.i < 0 || a.thr.i >= n)) return hipErrorInvalidValue;
    if (a.st ? (!a.atab || !a.htab || !a.coef || a.z) : (a.kx0 || a.pair_B > 0)) return hipErrorInvalidValue;
    if (a.kx0 && (!a.kmask || !a.ktab)) return hipErrorInvalidValue;
    bool vec = hw % 4 == 0;      // 16-byte accesses: every image then starts on a 16-byte boundary of an aligned buffer
    for (const void* p : {(const void*)a.x, (const void*)a.m, (const void*)a.z, (const void*)a.h, (const void*)a.out, (const void*)a.kx0,
                          (const void*)a.kmask})
        vec = vec && (uintptr_t)p % 16 == 0;
    if (vec) hipLaunchKernelGGL(threshold_step_kernel<4>, dim3(a.B), dim3(1024), 0, s, a);
    else hipLaunchKernelGGL(threshold_step_kernel<1>, dim3(a.B), dim3(1024), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_ee_select(const float* outs, const float* eps, const float* cls, float thr, int depth, int B, long long chw,
                            float* mo, int* idx, float* err_mean, hipStream_t s) {
    const long long n = (long long)B * chw;
    hipLaunchKernelGGL(ee_select_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, outs, eps, cls, thr, depth, B, chw, mo, idx);
    if (err_mean) hipLaunchKernelGGL(ee_batch_mean_kernel, dim3(depth), dim3(64), 0, s, cls, err_mean, B, (const StepState*)nullptr, 0.0f);
    return hipGetLastError();
}
hipError_t launch_ee_select_step(float* x, const float* outs, const float* eps, const float* cls, float thr, int depth, int* idx, float* err_mean,
                                 int idx_stride, int idx_col0, bool sums, StepState* st, const StepCoef* coef, int B, int C, int S,
                                 int noise_mode, int advance, hipStream_t s, const unsigned long long* seeds) {
    const long long npix = (long long)B * S * S;
    if (err_mean) hipLaunchKernelGGL(ee_batch_mean_kernel, dim3(depth), dim3(64), 0, s, cls, err_mean, B, st, sums ? 1.0f : 0.0f);
    hipLaunchKernelGGL(ee_select_step_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, x, outs, eps, cls, thr, depth, idx,
                       idx_stride > 0 ? idx_stride : B, idx_col0, st, coef, B, C, S, noise_mode, advance, idx_col0, seeds);
    return hipGetLastError();
}
hipError_t launch_noise_images(float* out, const unsigned long long* seeds, unsigned long long seed, int ctr, int B, int C, int S, hipStream_t s) {
    const long long hw = (long long)S * S;
    if (!out || B < 1 || C < 1 || C > 4 || S < 1 || hw > (1ll << 30) || ctr < 0) return hipErrorInvalidValue;
    const bool vec = hw % 4 == 0 && (uintptr_t)out % 16 == 0;
    const long long threads = (long long)B * (vec ? hw / 4 : hw), blocks = (threads + 255) / 256;
    if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
    if (vec) hipLaunchKernelGGL(noise_images_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, s, out, seeds, seed, ctr, B, C, (int)hw);
    else hipLaunchKernelGGL(noise_images_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, s, out, seeds, seed, ctr, B, C, (int)hw);
    return hipGetLastError();
}
hipError_t launch_ee_mean_combine(const float* s0, const float* s1, float* err, int depth, int t_lo, int t_hi, int B, hipStream_t s) {
    const int n = (t_hi - t_lo + 1) * depth;
    hipLaunchKernelGGL(ee_mean_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, s0, s1, err, depth, t_lo, t_hi, B);
    return hipGetLastError();
}
hipError_t launch_set_state(StepState* st, int t, unsigned long long seed, hipStream_t s) {
    hipLaunchKernelGGL(set_state_kernel, dim3(1), dim3(1), 0, s, st, t, seed);
    return hipGetLastError();
}
hipError_t launch_set_state_table(StepState* st, const AffineRow* atab, unsigned long long seed, hipStream_t s) {
    hipLaunchKernelGGL(set_state_table_kernel, dim3(1), dim3(1), 0, s, st, atab, seed);
    return hipGetLastError();
}
hipError_t launch_guided_labels(const long long* y, long long* out, int B, long long null_label, hipStream_t s) {
    hipLaunchKernelGGL(guided_labels_kernel, dim3((unsigned)((2 * B + 255) / 256)), dim3(256), 0, s, y, out, B, null_label);
    return hipGetLastError();
}
hipError_t launch_set_state_float(StepState* st, float t, hipStream_t s) {
    hipLaunchKernelGGL(set_state_float_kernel, dim3(1), dim3(1), 0, s, st, t);
    return hipGetLastError();
}
hipError_t launch_to_images(const float* x, float* out, int B, int C, int S, hipStream_t s) {
    const long long npix = (long long)B * S * S;
    hipLaunchKernelGGL(to_images_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, x, out, B, C, S);
    return hipGetLastError();
}

}  // namespace dd
