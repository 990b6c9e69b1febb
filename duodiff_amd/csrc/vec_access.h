// W consecutive floats of global or LDS memory in one access (device only): W = 4 a 16-byte load / store (the address 16-byte aligned),
// W = 1 a plain one.  The elementwise step kernels (step.hip, jump.hip) take W = 4 where the image size and the pointers allow.
#pragma once
#include "dd_internal.h"

namespace dd {

template <int W>
__device__ __forceinline__ void load_w(float (&d)[W], const float* p) {
    if constexpr (W == 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p);
        d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
    } else {
        d[0] = *p;
    }
}
template <int W>
__device__ __forceinline__ void store_w(float* p, const float (&d)[W]) {
    if constexpr (W == 4) *reinterpret_cast<f32x4*>(p) = f32x4{d[0], d[1], d[2], d[3]};
    else *p = d[0];
}
// component c of a four-channel draw
__device__ __forceinline__ float pick(const f32x4& v, int c) { return c == 0 ? v[0] : c == 1 ? v[1] : c == 2 ? v[2] : v[3]; }

}  // namespace dd
