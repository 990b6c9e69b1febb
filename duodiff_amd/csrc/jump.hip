// The resampling jump of the table-driven loops (gfx950): RePaint's resampling and Restart sampling go back up the timestep grid by forward
// noising, with no model evaluation.  The jump kernel of the device loop (dd_sample_affine_walk), its one-thread advance and the unfused rule
// (dd_jump_step).  The rule itself is defined in step_update.h beside the step update.  A unit of its own: the step kernels' unit holds none
// of it.  All arithmetic is fp32.
#include "dd_internal.h"
#include "step_update.h"
#include "vec_access.h"

namespace dd {
namespace {

// A resampling jump of a table-driven loop (step_update.h jump; dd_sample_affine_walk), in place on a chain's B images x [B, C, S, S]: row
// k = st->t of the table holds (a, c) = (ja, jc), and z3 is the Philox draw at draw_site's (key, id) of the pixel (b0: the chain's first image
// within the whole batch; seeds: the whole batch's staged per-image seeds or null), the row's counter and the stream word PHILOX_JUMP -- drawn
// where the row says noise and the loop draws on the device at all.  One draw serves a pixel's channels.  A thread owns W consecutive pixels
// of one image: W = 4 where hw % 4 == 0 and x is 16-byte aligned (16-byte accesses), else W = 1.  pair > 0 (classifier-free guidance): x'
// goes to the twin image too, `pair` elements on.  Every workgroup reads st->t, so no thread of this launch moves it: jump_advance_kernel,
// one thread behind it on the stream, hands the next row its index and t_model the way StepRule::advance does.
template <int W>
__global__ void __launch_bounds__(256) jump_kernel(float* x, const StepState* __restrict__ st, const AffineRow* __restrict__ atab,
                                                   const unsigned long long* __restrict__ seeds, int B, int C, int hw, int b0, long long pair,
                                                   int noise_mode) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int per_image = hw / W;
    if (i >= (long long)B * per_image) return;
    const AffineRow row = atab[st->t];
    const bool draw = noise_mode == 2 && row.noise != 0;
    const long long b = i / per_image;
    const int p0 = (int)(i - b * per_image) * W;
    f32x4 zn[W];
#pragma unroll
    for (int w = 0; w < W; ++w) {
        zn[w] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (draw) {
            const DrawSite ds = draw_site(seeds, st->seed, (unsigned long long)(b + b0), (unsigned long long)(p0 + w), (unsigned long long)hw);
            zn[w] = philox_normal4(ds.key, ds.id, row.ctr, PHILOX_JUMP);
        }
    }
    for (int c = 0; c < C; ++c) {
        float* px = x + (b * C + c) * hw + p0;
        float v[W];
        load_w<W>(v, px);
#pragma unroll
        for (int w = 0; w < W; ++w) v[w] = jump(v[w], pick(zn[w], c), row.a, row.c, draw);
        store_w<W>(px, v);
        if (pair > 0) store_w<W>(px + pair, v);
    }
}
__global__ void jump_advance_kernel(StepState* st, const AffineRow* __restrict__ atab) {
    const int tn = st->t + 1;
    st->t = tn;
    st->t_model = atab[tn].t_model;
}

// the unfused jump on n elements from a caller's z3 (dd_jump_step); x and out may alias.  W = 4: thread i owns elements [4 i, 4 i + 4), the
// whole groups with 16-byte accesses and the last, partial one element by element (x, z, out 16-byte aligned); W = 1: one element each.
template <int W>
__global__ void __launch_bounds__(256) jump_step_kernel(const float* x, const float* __restrict__ z, float* out, float ja, float jc, long long n) {
#pragma clang fp contract(off)
    const long long e0 = ((long long)blockIdx.x * 256 + threadIdx.x) * W;
    if (e0 >= n) return;
    if constexpr (W == 4) {
        if (e0 + 4 <= n) {
            float xv[4], zv[4] = {0.f, 0.f, 0.f, 0.f};
            load_w<4>(xv, x + e0);
            if (z) load_w<4>(zv, z + e0);
#pragma unroll
            for (int w = 0; w < 4; ++w) xv[w] = jump(xv[w], zv[w], ja, jc, z != nullptr);
            store_w<4>(out + e0, xv);
            return;
        }
    }
    for (long long e = e0; e < n && e < e0 + W; ++e) out[e] = jump(x[e], z ? z[e] : 0.f, ja, jc, z != nullptr);
}

}  // namespace

hipError_t launch_jump(float* x, StepState* st, const AffineRow* atab, const unsigned long long* seeds, int B, int C, int S, int b0, int pair_B,
                       int noise_mode, hipStream_t s) {
    const long long hw = (long long)S * S;
    if (!x || !st || !atab || B < 1 || C < 1 || C > 4 || S < 1 || hw > (1ll << 30) || b0 < 0 || pair_B < 0) return hipErrorInvalidValue;
    const bool vec = hw % 4 == 0 && (uintptr_t)x % 16 == 0;      // (then every image, the twins included, starts on a 16-byte boundary)
    const long long threads = (long long)B * (vec ? hw / 4 : hw), blocks = (threads + 255) / 256, pair = (long long)pair_B * C * hw;
    if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
    if (vec) hipLaunchKernelGGL(jump_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, s, x, st, atab, seeds, B, C, (int)hw, b0, pair, noise_mode);
    else hipLaunchKernelGGL(jump_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, s, x, st, atab, seeds, B, C, (int)hw, b0, pair, noise_mode);
    hipLaunchKernelGGL(jump_advance_kernel, dim3(1), dim3(1), 0, s, st, atab);
    return hipGetLastError();
}
hipError_t launch_jump_step(const float* x, const float* z, float* out, float ja, float jc, long long n, hipStream_t s) {
    if (!x || !out || n < 1) return hipErrorInvalidValue;
    const bool vec = (uintptr_t)x % 16 == 0 && (uintptr_t)z % 16 == 0 && (uintptr_t)out % 16 == 0;
    const long long threads = vec ? (n + 3) / 4 : n, blocks = (threads + 255) / 256;
    if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
    if (vec) hipLaunchKernelGGL(jump_step_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, s, x, z, out, ja, jc, n);
    else hipLaunchKernelGGL(jump_step_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, s, x, z, out, ja, jc, n);
    return hipGetLastError();
}

}  // namespace dd
