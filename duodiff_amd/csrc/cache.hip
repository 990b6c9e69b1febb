// Block caching (gfx950): the deep blocks' output y_deep is kept across sampling steps (DeepCache, Ma et al. 2024) and a reuse step feeds the
// long-skip path a cached copy of it -- or, order 1, a linear extrapolation of the last two (TaylorSeer).  This unit holds the one kernel of
// the feature: y^ = last + w (last - prev) on a chain's [rows L, D] cache, in the activation type.  The forward that reads y^ is forward.hip's.
#include "dd_internal.h"

#include <algorithm>

namespace dd {
namespace {

// One 16-byte group of T per lane and pass: 8 bf16 or 4 fp32.
template <typename T> struct Group;
template <> struct Group<bf16_t> { typedef bf16x8 vec; static constexpr int n = 8; };
template <> struct Group<float> { typedef f32x4 vec; static constexpr int n = 4; };

// out = last + w (last - prev) on ngroups 16-byte groups (n = rows L D elements, a multiple of 64 as D % 64 == 0), fp32 arithmetic:
// d = last - prev; y = last + w d, contraction off, rounded once to T.  The op and w come from row st->t of the step table where atab is set
// (pad1 = the op, pad2 = the bits of w: a captured step replays for every row) and from the arguments otherwise.  op 2 extrapolates; any other
// op copies last and never reads prev (0 * NaN is NaN: a row without a prev is chosen by its op, not by w = 0).  No thread of a step writes
// st->t before the step's last kernel, which is behind this one on the stream.  out aliases neither input.
template <typename T>
__global__ void __launch_bounds__(256) cache_extrapolate_kernel(const T* __restrict__ last, const T* __restrict__ prev, T* __restrict__ out,
                                                                long long ngroups, const StepState* __restrict__ st,
                                                                const AffineRow* __restrict__ atab, int op_arg, float w_arg) {
#pragma clang fp contract(off)
    typedef typename Group<T>::vec vec;
    constexpr int G = Group<T>::n;
    int op = op_arg;
    float w = w_arg;
    if (atab) {
        const AffineRow row = atab[st->t];
        op = row.pad1;
        w = __builtin_bit_cast(float, row.pad2);
    }
    const bool extrapolate = op == 2;
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < ngroups; i += stride) {
        const vec l = reinterpret_cast<const vec*>(last)[i];
        vec o = l;
        if (extrapolate) {
            const vec p = reinterpret_cast<const vec*>(prev)[i];
#pragma unroll
            for (int j = 0; j < G; ++j) {
                float lf, pf;
                if constexpr (sizeof(T) == 2) { lf = bf2f((bf16_t)l[j]); pf = bf2f((bf16_t)p[j]); }
                else { lf = l[j]; pf = p[j]; }
                const float d = lf - pf;
                const float y = lf + w * d;
                if constexpr (sizeof(T) == 2) o[j] = (short)f2bf(y);
                else o[j] = y;
            }
        }
        reinterpret_cast<vec*>(out)[i] = o;
    }
}

}  // namespace

// n elements of the activation type (bf16: 2 bytes, else fp32), n % 64 == 0 and the three buffers 16-byte aligned; prev may be null where no
// row of the launch extrapolates (atab null and op != 2).  The grid is capped at 2048 workgroups and strided.
hipError_t launch_cache_extrapolate(const void* last, const void* prev, void* out, long long n, bool bf16, const StepState* st,
                                    const AffineRow* atab, int op, float w, hipStream_t s) {
    if (!last || !out || n < 64 || n % 64 || last == out || prev == out || (atab && !st) || ((atab || op == 2) && !prev)) return hipErrorInvalidValue;
    if ((uintptr_t)last % 16 || (uintptr_t)prev % 16 || (uintptr_t)out % 16) return hipErrorInvalidValue;
    const long long ngroups = n / (bf16 ? 8 : 4);
    const unsigned blocks = (unsigned)std::min<long long>((ngroups + 255) / 256, CACHE_MAX_BLOCKS);
    if (bf16)
        hipLaunchKernelGGL(cache_extrapolate_kernel<bf16_t>, dim3(blocks), dim3(256), 0, s, (const bf16_t*)last, (const bf16_t*)prev, (bf16_t*)out,
                           ngroups, st, atab, op, w);
    else
        hipLaunchKernelGGL(cache_extrapolate_kernel<float>, dim3(blocks), dim3(256), 0, s, (const float*)last, (const float*)prev, (float*)out,
                           ngroups, st, atab, op, w);
    return hipGetLastError();
}

}  // namespace dd
