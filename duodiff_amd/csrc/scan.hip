// The denoising-error scan (gfx950): real images noised to a chosen timestep in front of the model, and the model's error against the
// training target behind it (dd_scan_error; reference trainer.py:307-352 at one timestep).  Two kernels around forward_eps, in the
// step-state contract of dd_internal.h: scan_diffuse_kernel is a step's first kernel and reads row st->t, token assembly copies t to
// t_final, scan_error_kernel is its last, reads row t_final, and one of its threads hands the next step its t / t_model.  All arithmetic
// is step_update.h's (draw_site, philox_normal4, known_value, scan_target, scan_accumulate, scan_mean): the kernels hold none of their own.
// Both are launch-latency sized (a few MB each way at the largest batch).
#include "dd_internal.h"
#include "step_update.h"
#include "wave_prims.h"

namespace dd {
namespace {

// x_t = ka x0 + kb z for B images.  A thread owns a pixel and its C channels: one philox_normal4 call serves them all (as the known
// region's z2 in step.hip), and consecutive lanes touch consecutive pixels of one channel plane, so every access is coalesced.
template <int C>
__global__ void __launch_bounds__(256) scan_diffuse_kernel(const float* __restrict__ x0, float* __restrict__ xt, const StepState* __restrict__ st,
                                                           const ScanRow* __restrict__ tab, const unsigned long long* __restrict__ seeds,
                                                           int B, int hw, int b0) {
    const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
    if (pix >= (long long)B * hw) return;
    const ScanRow row = tab[st->t];
    const long long b = pix / hw, p = pix - b * hw;
    const DrawSite ds = draw_site(seeds, st->seed, (unsigned long long)(b + b0), (unsigned long long)p, (unsigned long long)hw);
    const f32x4 z = philox_normal4(ds.key, ds.id, row.ctr, PHILOX_SCAN);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const long long e = (b * C + c) * hw + p;
        xt[e] = known_value(x0[e], row.ka, row.kb, z[c], true);
    }
}

// err[t B_all + b0 + b] = (1 / CHW) sum (m - tgt)^2 of image b: one workgroup of 256 threads per image.  z is drawn again from the same site
// and counter (there is no z buffer) and x_t recomputed by the same known_value: bit for bit what the model saw.  The sum is taken in fp32
// in an order fixed by (C, S) alone:
//   1. thread tid adds its pixels p = tid, tid + 256, ..., channels 0 .. C - 1 of each, left to right:  C ceil(S S / 256) terms
//   2. wave_reduce_add over the wave's 64 lanes (a butterfly: 6 levels)
//   3. the 4 waves' sums through LDS, added in wave order by thread 0 (3 adds)
// SUMMATION DEPTH: no term passes through more than  C ceil(S S / 256) + 6 + 3  additions; then one division by C S S.
template <int C>
__global__ void __launch_bounds__(256) scan_error_kernel(const float* __restrict__ x0, const float* __restrict__ m, float* __restrict__ err,
                                                         StepState* st, const ScanRow* __restrict__ tab,
                                                         const unsigned long long* __restrict__ seeds, int hw, int b0, int B_all, int advance) {
    __shared__ float part[4];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int k = st->t_final;
    const ScanRow row = tab[k];
    const float t_next = advance ? tab[k + 1].t_model : 0.f;
    const unsigned long long seed = st->seed;
    float acc = 0.f;
    for (int p = tid; p < hw; p += 256) {
        const DrawSite ds = draw_site(seeds, seed, (unsigned long long)(b + b0), (unsigned long long)p, (unsigned long long)hw);
        const f32x4 z = philox_normal4(ds.key, ds.id, row.ctr, PHILOX_SCAN);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const long long e = ((long long)b * C + c) * hw + p;
            const float xv = x0[e];
            const float xt = known_value(xv, row.ka, row.kb, z[c], true);
            acc = scan_accumulate(acc, m[e], scan_target(z[c], xv, xt, row.tz, row.t0, row.tx));
        }
    }
    acc = wave_reduce_add(acc);
    if ((tid & 63) == 0) part[tid >> 6] = acc;
    __syncthreads();
    if (tid != 0) return;
    float sum = part[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) sum += part[w];
    err[(long long)k * B_all + b0 + b] = scan_mean(sum, C * hw);
    if (b == 0 && advance) {      // (no workgroup reads t / t_model: they read t_final)
        st->t = k + 1;
        st->t_model = t_next;
    }
}

__global__ void set_state_scan_kernel(StepState* st, const ScanRow* tab, unsigned long long seed) {
    st->t = 0;
    st->t_final = 0;
    st->t_model = tab[0].t_model;
    st->seed = seed;
}

bool scan_shape_ok(int B, int C, int S) {
    return B >= 1 && C >= 1 && C <= 4 && S >= 1 && (long long)S * S * C <= (1ll << 24);
}

}  // namespace

hipError_t launch_scan_diffuse(const float* x0, float* xt, const StepState* st, const ScanRow* tab, const unsigned long long* seeds, int B, int C,
                               int S, int b0, hipStream_t s) {
    if (!scan_shape_ok(B, C, S) || !x0 || !xt || !st || !tab || b0 < 0) return hipErrorInvalidValue;
    const int hw = S * S;
    const long long blocks = ((long long)B * hw + 255) / 256;
    if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, s, x0, xt, st, tab, seeds, B, hw, b0); };
    if (C == 1) go(scan_diffuse_kernel<1>);
    else if (C == 2) go(scan_diffuse_kernel<2>);
    else if (C == 3) go(scan_diffuse_kernel<3>);
    else go(scan_diffuse_kernel<4>);
    return hipGetLastError();
}

hipError_t launch_scan_error(const float* x0, const float* m, float* err, StepState* st, const ScanRow* tab, const unsigned long long* seeds,
                             int B, int C, int S, int b0, int B_all, int advance, hipStream_t s) {
    if (!scan_shape_ok(B, C, S) || !x0 || !m || !err || !st || !tab || b0 < 0 || B_all < b0 + B) return hipErrorInvalidValue;
    const int hw = S * S;
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(256), 0, s, x0, m, err, st, tab, seeds, hw, b0, B_all, advance); };
    if (C == 1) go(scan_error_kernel<1>);
    else if (C == 2) go(scan_error_kernel<2>);
    else if (C == 3) go(scan_error_kernel<3>);
    else go(scan_error_kernel<4>);
    return hipGetLastError();
}

hipError_t launch_set_state_scan(StepState* st, const ScanRow* tab, unsigned long long seed, hipStream_t s) {
    hipLaunchKernelGGL(set_state_scan_kernel, dim3(1), dim3(1), 0, s, st, tab, seed);
    return hipGetLastError();
}

}  // namespace dd
