// The denoising-error scan (gfx950): real images noised to a chosen timestep in front of the model, and the model's error against the
// training target behind it (dd_scan_error; reference trainer.py:307-352 at one timestep).  Two kernels around forward_eps, in the
// step-state contract of dd_internal.h: scan_diffuse_kernel is a step's first kernel and reads row st->t, token assembly copies t to
// t_final, scan_error_kernel is its last, reads row t_final, and one of its threads hands the next step its t / t_model.  All arithmetic
// is step_update.h's (draw_site, philox_normal4, known_value, scan_target, scan_accumulate, scan_mean): the kernels hold none of their own.
// Both are launch-latency sized (a few MB each way at the largest batch).  dd_scan_error_early_exit keeps the diffuse kernel and ends its
// step with scan_exits_error_kernel: every exit's error and the probes' training target from one forward's taps.  The two error kernels
// keep their own row lookup, output index and hand-off and share one summation (scan_image_sums, scan_sum_waves); the three launchers
// share one channel dispatch (with_channels).
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

// The one summation of both error kernels, in the order stated above scan_error_kernel.  scan_image_sums: steps 1 and 2 for image b of the
// launch against the plane m, the wave sums left in part[0][0 .. 3] behind a barrier (TANH: the sum of scan_accumulate_tanh too, term for
// term beside the squares, in part[1]).  scan_sum_waves: step 3 on one such row.
template <int C, bool TANH>
__device__ __forceinline__ void scan_image_sums(const float* __restrict__ x0, const float* __restrict__ m, const ScanRow& row,
                                                const unsigned long long* __restrict__ seeds, unsigned long long seed, int b, int b0, int hw,
                                                float (*part)[4]) {
    const int tid = threadIdx.x;
    float acc = 0.f, acu = 0.f;
    for (int p = tid; p < hw; p += 256) {
        const DrawSite ds = draw_site(seeds, seed, (unsigned long long)(b + b0), (unsigned long long)p, (unsigned long long)hw);
        const f32x4 z = philox_normal4(ds.key, ds.id, row.ctr, PHILOX_SCAN);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const long long e = ((long long)b * C + c) * hw + p;
            const float xv = x0[e];
            const float xt = known_value(xv, row.ka, row.kb, z[c], true);
            const float tgt = scan_target(z[c], xv, xt, row.tz, row.t0, row.tx);
            const float o = m[e];
            acc = scan_accumulate(acc, o, tgt);
            if constexpr (TANH) acu = scan_accumulate_tanh(acu, o, tgt);
        }
    }
    acc = wave_reduce_add(acc);
    if constexpr (TANH) acu = wave_reduce_add(acu);
    if ((tid & 63) == 0) {
        part[0][tid >> 6] = acc;
        if constexpr (TANH) part[1][tid >> 6] = acu;
    }
    __syncthreads();
}
__device__ __forceinline__ float scan_sum_waves(const float* part) {
    float sum = part[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) sum += part[w];
    return sum;
}

// err[t B_all + b0 + b] = (1 / CHW) sum (m - tgt)^2 of image b: one workgroup of 256 threads per image.  z is drawn again from the same site
// and counter (there is no z buffer) and x_t recomputed by the same known_value: bit for bit what the model saw.  The sum is taken in fp32
// in an order fixed by (C, S) alone:
//   1. thread tid adds its pixels p = tid, tid + 256, ..., channels 0 .. C - 1 of each, left to right:  C ceil(S S / 256) terms
//   2. wave_reduce_add over the wave's 64 lanes (a butterfly: 6 levels)
//   3. the 4 waves' sums through LDS, added in wave order by thread 0 (3 adds)
// SUMMATION DEPTH: no term passes through more than  C ceil(S S / 256) + 6 + 3  additions; then one division by C S S.
// The row table is indexed by the step (st->t_final = k); the handoff goes to row k + 1.
template <int C>
__global__ void __launch_bounds__(256) scan_error_kernel(const float* __restrict__ x0, const float* __restrict__ m, float* __restrict__ err,
                                                         StepState* st, const ScanRow* __restrict__ tab,
                                                         const unsigned long long* __restrict__ seeds, int hw, int b0, int B_all, int advance) {
    __shared__ float part[1][4];
    const int b = blockIdx.x;
    const int k = st->t_final;
    const ScanRow row = tab[k];
    const float t_next = advance ? tab[k + 1].t_model : 0.f;
    scan_image_sums<C, false>(x0, m, row, seeds, st->seed, b, b0, hw, part);
    if (threadIdx.x != 0) return;
    err[(long long)k * B_all + b0 + b] = scan_mean(scan_sum_waves(part[0]), C * hw);
    if (b == 0 && advance) {      // (no workgroup reads t / t_model: they read t_final)
        st->t = k + 1;
        st->t_model = t_next;
    }
}

// The early-exit form (dd_scan_error_early_exit): one forward's E = depth + 1 outputs against the one target.  Exit l < E - 1 reads plane l
// of outs [E - 1, B, C, S, S], exit E - 1 the backbone's eps; workgroup (b, l) takes image b and exit l: scan_error_kernel with blockIdx.y
// over the exits and a second accumulator.  Both sums are scan_image_sums' and scan_sum_waves', so mse[k][l] is bit-equal to
// scan_error_kernel on plane l and the SUMMATION DEPTH above holds for both.  Consecutive lanes read consecutive pixels of one plane.
//   mse [k][l][b0 + b] = scan_mean(sum scan_accumulate(., o_l, tgt))         k = row.ctr - tab[1000].ctr, the step's index in the call
//   tgtu[k][l][b0 + b] = scan_mean(sum scan_accumulate_tanh(., o_l, tgt))    the probes' training target (trainer.py:376)
//   pred[k][l][b0 + b] = cls[l][b]  (l < E - 1)                              what the probes predicted: a copy
// The row table is indexed by the TIMESTEP here (st->t_final is the integer timestep, which the per-timestep probe tables of the forward
// need): rows 0 .. 999, and row SCAN_EXITS_ROWS = 1000 whose ctr is the call's counter_base; the handoff goes to row `next`.
// One exit per workgroup is the measured choice (tools/scan_exits_bench.py; 64 images of 3 x 64 x 64, 14 exits, the launch alone).  A form
// that drew z and formed tgt once per pixel for a group of G exits (accumulators in registers, the exit loop inside the pixel loop) took
// 84.6 us at G = 4, 54.6 us at G = 2 and 41.8 us at G = 1 against 37.9 us for this kernel, and 151 us for 14 launches of scan_error_kernel: the summation order
// fixes 256 threads per (image, exit), so the launch has 3.5 waves per SIMD here and under one at G = 4, and the waves that hide the
// planes' load latency are worth more than the Philox draws that grouping saves.  The grouped form is not in this tree.
template <int C>
__global__ void __launch_bounds__(256) scan_exits_error_kernel(const float* __restrict__ x0, const float* __restrict__ outs, const float* __restrict__ eps,
                                                               const float* __restrict__ cls, float* __restrict__ mse, float* __restrict__ tgtu,
                                                               float* __restrict__ pred, StepState* st, const ScanRow* __restrict__ tab,
                                                               const unsigned long long* __restrict__ seeds, int hw, int b0, int B, int B_all, int E,
                                                               int advance) {
    __shared__ float part[2][4];
    const int tid = threadIdx.x, b = blockIdx.x, l = blockIdx.y;
    const int t = st->t_final;
    const ScanRow row = tab[t];
    const int k = row.ctr - tab[SCAN_EXITS_ROWS].ctr;      // (the call's counter_base: device data, so a captured step serves every base)
    const float t_next = advance ? tab[row.next].t_model : 0.f;
    scan_image_sums<C, true>(x0, l < E - 1 ? outs + (long long)l * B * C * hw : eps, row, seeds, st->seed, b, b0, hw, part);
    if (tid < 2) {       // thread 0: the squares, thread 1: the tanh sum
        (tid ? tgtu : mse)[((long long)k * E + l) * B_all + b0 + b] = scan_mean(scan_sum_waves(part[tid]), C * hw);
        if (tid == 0 && l < E - 1) pred[((long long)k * (E - 1) + l) * B_all + b0 + b] = cls[(long long)l * B + b];
    }
    if (tid == 0 && b == 0 && l == 0 && advance) {      // (no workgroup reads t / t_model: they read t_final)
        st->t = row.next;
        st->t_model = t_next;
    }
}

__global__ void set_state_scan_kernel(StepState* st, const ScanRow* tab, unsigned long long seed, int row) {
    st->t = row;
    st->t_final = row;
    st->t_model = tab[row].t_model;
    st->seed = seed;
}

bool scan_shape_ok(int B, int C, int S) {
    return B >= 1 && C >= 1 && C <= 4 && S >= 1 && (long long)S * S * C <= (1ll << 24);
}

// f(integral_constant<int, C>) for the channel count of a launch (scan_shape_ok: 1..4): the one place a kernel's C is chosen
template <typename F>
void with_channels(int C, F&& f) {
    if (C == 1) f(std::integral_constant<int, 1>{});
    else if (C == 2) f(std::integral_constant<int, 2>{});
    else if (C == 3) f(std::integral_constant<int, 3>{});
    else f(std::integral_constant<int, 4>{});
}

}  // namespace

hipError_t launch_scan_diffuse(const float* x0, float* xt, const StepState* st, const ScanRow* tab, const unsigned long long* seeds, int B, int C,
                               int S, int b0, hipStream_t s) {
    if (!scan_shape_ok(B, C, S) || !x0 || !xt || !st || !tab || b0 < 0) return hipErrorInvalidValue;
    const int hw = S * S;
    const long long blocks = ((long long)B * hw + 255) / 256;
    if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
    with_channels(C, [&](auto c) {
        hipLaunchKernelGGL(scan_diffuse_kernel<decltype(c)::value>, dim3((unsigned)blocks), dim3(256), 0, s, x0, xt, st, tab, seeds, B, hw, b0);
    });
    return hipGetLastError();
}

hipError_t launch_scan_error(const float* x0, const float* m, float* err, StepState* st, const ScanRow* tab, const unsigned long long* seeds,
                             int B, int C, int S, int b0, int B_all, int advance, hipStream_t s) {
    if (!scan_shape_ok(B, C, S) || !x0 || !m || !err || !st || !tab || b0 < 0 || B_all < b0 + B) return hipErrorInvalidValue;
    const int hw = S * S;
    with_channels(C, [&](auto c) {
        hipLaunchKernelGGL(scan_error_kernel<decltype(c)::value>, dim3((unsigned)B), dim3(256), 0, s, x0, m, err, st, tab, seeds, hw, b0, B_all, advance);
    });
    return hipGetLastError();
}

hipError_t launch_scan_exits_error(const float* x0, const float* outs, const float* eps, const float* cls, float* mse, float* tgtu, float* pred,
                                   StepState* st, const ScanRow* tab, const unsigned long long* seeds, int B, int C, int S, int exits, int b0,
                                   int B_all, int advance, hipStream_t s) {
    if (!scan_shape_ok(B, C, S) || exits < 1 || exits > 32 || !x0 || !eps || !mse || !tgtu || !st || !tab || b0 < 0 || B_all < b0 + B)
        return hipErrorInvalidValue;
    if (exits > 1 && (!outs || !cls || !pred)) return hipErrorInvalidValue;
    const int hw = S * S;
    with_channels(C, [&](auto c) {
        hipLaunchKernelGGL(scan_exits_error_kernel<decltype(c)::value>, dim3((unsigned)B, (unsigned)exits), dim3(256), 0, s, x0, outs, eps, cls, mse, tgtu,
                           pred, st, tab, seeds, hw, b0, B, B_all, exits, advance);
    });
    return hipGetLastError();
}

hipError_t launch_set_state_scan(StepState* st, const ScanRow* tab, unsigned long long seed, hipStream_t s, int row) {
    hipLaunchKernelGGL(set_state_scan_kernel, dim3(1), dim3(1), 0, s, st, tab, seed, row);
    return hipGetLastError();
}

}  // namespace dd
