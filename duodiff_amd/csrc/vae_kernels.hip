// Bandwidth kernels of the KL-VAE decoder and encoder (reference models/utils/autoencoder.py:203-449): layout
// changes, im2col for the 3x3 convolutions (optionally through a nearest-2x upsample, or with the stride 2 of
// Downsample), GroupNorm(32) + swish, row softmax of the single-head attention block, quant_conv + the
// posterior sample.  All convolutions themselves run as GEMMs on the MFMA kernels of gemm.hip (NHWC
// activations: a pixel is a GEMM row).
#include "dd_internal.h"

namespace dd {
namespace {

__device__ __forceinline__ float block_sum_256(float v, float* sh) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}

// z [B,4,H,W] fp32 NCHW -> (1/scale) z -> post_quant_conv 1x1 (4->4, autoencoder.py:486-488) -> NHWC fp32 [B*H*W, 4]
__global__ void vae_input_kernel(const float* __restrict__ z, const float* __restrict__ w, const float* __restrict__ b,
                                 float inv_scale, float* __restrict__ out, int B, int HW) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)B * HW) return;
    const int bi = (int)(i / HW), p = (int)(i % HW);
    float v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = z[((long long)bi * 4 + c) * HW + p] * inv_scale;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        float a = b[o];
#pragma unroll
        for (int c = 0; c < 4; ++c) a = fmaf(w[o * 4 + c], v[c], a);
        out[i * 4 + o] = a;
    }
}

// NHWC fp32 [B*H*W, ldc] (first C channels) -> NCHW fp32 [B,C,H,W]
__global__ void vae_output_kernel(const float* __restrict__ in, float* __restrict__ out, int B, int C, int HW, int ldc) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)B * C * HW) return;
    const int p = (int)(i % HW), c = (int)((i / HW) % C), bi = (int)(i / ((long long)HW * C));
    out[i] = in[((long long)bi * HW + p) * ldc + c];
}

// im2col for a 3x3 / pad 1 convolution over NHWC `src` [B, Hs, Ws, C]; when up == 1 the convolution input is the
// nearest-2x upsampled image (autoencoder.py:56-59), gathered on the fly.  Row = output pixel, column order
// (ky, kx, c) (the weights are repacked to match), columns [9C, Kpad) are zero.  8 channels (16 B) per thread.
template <typename T>
__global__ void im2col3x3_kernel(const T* __restrict__ src, T* __restrict__ dst, int B, int H, int W, int C, int up,
                                 int Kpad) {
    constexpr int V = 16 / (int)sizeof(T);
    const int cv = C / V;                       // vectors per pixel (C % V == 0: the launcher refuses anything else)
    const long long per_row = (long long)Kpad / V;
    const long long total = (long long)B * H * W * per_row;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long long row = i / per_row;
    const int kc = (int)(i % per_row);
    f32x4 val = {0.f, 0.f, 0.f, 0.f};
    const int tap = kc / cv, c0 = (kc % cv) * V;
    if (tap < 9) {
        const int x = (int)(row % W), y = (int)((row / W) % H), bi = (int)(row / ((long long)W * H));
        const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
            const int Hs = up ? H / 2 : H, Ws = up ? W / 2 : W;
            const int ys = up ? yy / 2 : yy, xs = up ? xx / 2 : xx;
            val = *reinterpret_cast<const f32x4*>(src + (((long long)bi * Hs + ys) * Ws + xs) * C + c0);
        }
    }
    *reinterpret_cast<f32x4*>(dst + row * Kpad + (long long)kc * V) = val;
}

// im2col of Downsample (autoencoder.py:69-73): pad (0, 1, 0, 1) + 3x3 stride-2 convolution over NHWC `src` [B, 2H, 2W, C].  Row = output
// pixel (y, x) of the H x W result, which reads input rows 2y .. 2y + 2 and columns 2x .. 2x + 2; row 2H / column 2W is the zero pad and
// there is none on the top / left.  Columns as im2col3x3_kernel: (ky, kx, c), [9C, Kpad) zero, 16 B per thread.
template <typename T>
__global__ void im2col3x3_s2_kernel(const T* __restrict__ src, T* __restrict__ dst, int B, int H, int W, int C, int Kpad) {
    constexpr int V = 16 / (int)sizeof(T);
    const int cv = C / V;
    const long long per_row = (long long)Kpad / V;
    const long long total = (long long)B * H * W * per_row;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long long row = i / per_row;
    const int kc = (int)(i % per_row);
    f32x4 val = {0.f, 0.f, 0.f, 0.f};
    const int tap = kc / cv, c0 = (kc % cv) * V;
    if (tap < 9) {
        const int x = (int)(row % W), y = (int)((row / W) % H), bi = (int)(row / ((long long)W * H));
        const int yy = 2 * y + tap / 3, xx = 2 * x + tap % 3;
        if (yy < 2 * H && xx < 2 * W)
            val = *reinterpret_cast<const f32x4*>(src + (((long long)bi * 2 * H + yy) * 2 * W + xx) * C + c0);
    }
    *reinterpret_cast<f32x4*>(dst + row * Kpad + (long long)kc * V) = val;
}

// x [B,3,H,W] fp32 NCHW (an image in [-1, 1]) -> NHWC fp32 [B*H*W, 4], the fourth channel zero: the encoder's conv_in then gathers it
// with im2col3x3_c4_kernel (K = 36, the weight's fourth-channel columns zero)
__global__ void vae_image_kernel(const float* __restrict__ x, float* __restrict__ out, int B, int HW) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)B * HW) return;
    const int bi = (int)(i / HW), p = (int)(i % HW);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = x[((long long)bi * 3 + c) * HW + p];
    reinterpret_cast<f32x4*>(out)[i] = v;
}

// FrozenAutoencoderKL.sample (autoencoder.py:473-479) for one element: scale * (mean + exp(0.5 clamp(logvar, -30, 20)) eps), each
// product rounded on its own; exp is evaluated in double and rounded once (the correctly rounded fp32 exp).  use_eps false: the mode.
__device__ __forceinline__ float vae_sample_one(float mean, float logvar, float eps, bool use_eps) {
#pragma clang fp contract(off)
    if (!use_eps) return 0.18215f * mean;
    const float lv = fminf(fmaxf(logvar, -30.0f), 20.0f);
    const float sd = (float)exp(0.5 * (double)lv);
    return 0.18215f * (mean + sd * eps);
}

// conv_out rows [B*HW, 8] fp32 -> quant_conv 1x1 (8 -> 8, autoencoder.py:468-471) -> moments [B,8,HW] NCHW and / or z [B,4,HW]
__global__ void vae_moments_kernel(const float* __restrict__ h, const float* __restrict__ w, const float* __restrict__ b,
                                   const float* __restrict__ eps, float* __restrict__ moments, float* __restrict__ z, int B, int HW) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)B * HW) return;
    const int bi = (int)(i / HW), p = (int)(i % HW);
    float v[8], m[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = h[i * 8 + c];
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        float a = b[o];
#pragma unroll
        for (int c = 0; c < 8; ++c) a = fmaf(w[o * 8 + c], v[c], a);
        m[o] = a;
    }
    if (moments) {
#pragma unroll
        for (int o = 0; o < 8; ++o) moments[((long long)bi * 8 + o) * HW + p] = m[o];
    }
    if (z) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const long long at = ((long long)bi * 4 + c) * HW + p;
            z[at] = vae_sample_one(m[c], m[4 + c], eps ? eps[at] : 0.f, eps != nullptr);
        }
    }
}

// z = sample(moments [B,8,HW]) alone, elementwise over [B,4,HW]
__global__ void vae_sample_kernel(const float* __restrict__ moments, const float* __restrict__ eps, float* __restrict__ z, int B, int HW) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)B * 4 * HW) return;
    const long long per = 4LL * HW;
    const long long bi = i / per, r = i % per;
    z[i] = vae_sample_one(moments[bi * 2 * per + r], moments[bi * 2 * per + per + r], eps ? eps[i] : 0.f, eps != nullptr);
}

// conv_in has C = 4 input channels: K = 36, padded to Kpad; scalar gather
template <typename T>
__global__ void im2col3x3_c4_kernel(const float* __restrict__ src, T* __restrict__ dst, int B, int H, int W, int Kpad) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = (long long)B * H * W * Kpad;
    if (i >= total) return;
    const long long row = i / Kpad;
    const int k = (int)(i % Kpad);
    float v = 0.f;
    if (k < 36) {
        const int tap = k / 4, c = k % 4;
        const int x = (int)(row % W), y = (int)((row / W) % H), bi = (int)(row / ((long long)W * H));
        const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) v = src[(((long long)bi * H + yy) * W + xx) * 4 + c];
    }
    dst[i] = Elem<T>::from_f32(v);
}

// GroupNorm(32 groups, eps 1e-6) in three deterministic passes over the NHWC fp32 stream:
//   gn_stats    one workgroup per (image, chunk of kGnChunk pixels): per-group (sum, sum of squares) partials of d = x - pivot, fp32,
//               16-byte loads (a float4 = 4 channels of one group since C/32 >= 4), fixed-order LDS reduction;
//   gn_finalize one thread per (image, group): partials combined in double -> (mean, rstd) = (pivot + s / n, q / n - (s / n)^2);
//   gn_apply    y = swish?((x - mean) * rstd * gamma + beta) -> T, 16-byte loads.
// The pivot of an (image, group) is the group's first channel at the image's first pixel: a value of the group itself, so d is of the
// order of the group's spread and q / n - (s / n)^2 does not cancel however far the group's mean lies from zero (the sums of x and x^2
// lose (mean / std)^2 ulps in fp32, which the double of the finalize cannot give back); a constant group has d = 0 and var = 0 exactly.
// It depends on the image alone, as every partial does: an image normalises the same in any batch.
constexpr int kGnChunk = 256;
__global__ void __launch_bounds__(256) gn_stats_kernel(const float* __restrict__ x, float* __restrict__ part, int HW,
                                                       int C, int chunks) {
    __shared__ float ss[256], sq[256];
    const int bi = blockIdx.x / chunks, ch = blockIdx.x % chunks;
    const int c4 = C >> 2;                       // float4 columns per pixel: 32, 64 or 128
    const int rows = 256 / c4;                   // pixels covered per pass
    const int col = threadIdx.x % c4, r0 = threadIdx.x / c4;
    const int p0 = ch * kGnChunk, p1 = min(HW, p0 + kGnChunk);
    const float* xi = x + (long long)bi * HW * C;
    const float pv = xi[(col / (c4 >> 5)) * (C >> 5)];      // the pivot of this column's group
    const f32x4* xp = reinterpret_cast<const f32x4*>(xi) + col;
    f32x4 s = {0.f, 0.f, 0.f, 0.f}, q = {0.f, 0.f, 0.f, 0.f};
    for (int p = p0 + r0; p < p1; p += rows) {
        const f32x4 v = xp[(long long)p * c4] - pv;
        s += v;
        q += v * v;
    }
    ss[threadIdx.x] = (s[0] + s[1]) + (s[2] + s[3]);
    sq[threadIdx.x] = (q[0] + q[1]) + (q[2] + q[3]);
    __syncthreads();
    if (threadIdx.x < 32) {                      // group g owns float4 columns [g*w, (g+1)*w), w = c4/32
        const int w = c4 >> 5;
        float a = 0.f, b2 = 0.f;
        for (int r = 0; r < rows; ++r)
            for (int k = 0; k < w; ++k) {
                const int t = r * c4 + threadIdx.x * w + k;
                a += ss[t];
                b2 += sq[t];
            }
        float* o = part + (((long long)bi * chunks + ch) * 32 + threadIdx.x) * 2;
        o[0] = a;
        o[1] = b2;
    }
}

__global__ void gn_finalize_kernel(const float* __restrict__ x, const float* __restrict__ part, float* __restrict__ stat,
                                   int n_img_groups, int chunks, int HW, int C, double count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;   // (image, group)
    if (i >= n_img_groups) return;
    const int bi = i >> 5, g = i & 31;
    double s = 0.0, q = 0.0;
    for (int k = 0; k < chunks; ++k) {
        const float* o = part + (((long long)bi * chunks + k) * 32 + g) * 2;
        s += o[0];
        q += o[1];
    }
    const double ds = s / count;                           // mean - pivot
    double var = q / count - ds * ds;
    var = var > 0.0 ? var : 0.0;
    stat[2 * i] = (float)((double)x[(long long)bi * HW * C + g * (C >> 5)] + ds);
    stat[2 * i + 1] = (float)(1.0 / sqrt(var + 1e-6));
}

template <typename T>
__global__ void __launch_bounds__(256) gn_apply_kernel(const float* __restrict__ x, const float* __restrict__ stat,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       T* __restrict__ out, int HW, int C, int swish, long long total4) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // float4 index
    if (i >= total4) return;
    const int c4 = C >> 2;
    const int col = (int)(i % c4);
    const int bi = (int)(i / ((long long)HW * c4));
    const int g = col / (c4 >> 5);
    const float mean = stat[2 * (bi * 32 + g)], rstd = stat[2 * (bi * 32 + g) + 1];
    const f32x4 xv = reinterpret_cast<const f32x4*>(x)[i];
    const f32x4 ga = reinterpret_cast<const f32x4*>(gamma)[col], be = reinterpret_cast<const f32x4*>(beta)[col];
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float t = (xv[e] - mean) * rstd * ga[e] + be[e];
        if (swish) t = t / (1.0f + expf(-t));   // x * sigmoid(x)  (autoencoder.py:33-35)
        v[e] = t;
    }
    if constexpr (sizeof(T) == 4) {
        reinterpret_cast<f32x4*>(out)[i] = v;
    } else {
        T o4[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) o4[e] = Elem<T>::from_f32(v[e]);
        reinterpret_cast<uint2*>(out)[i] = *reinterpret_cast<const uint2*>(o4);
    }
}

// softmax over the last dim of S [rows, n] fp32 with a pre-scale; one wave per row; T out
template <typename T>
__global__ void __launch_bounds__(256) softmax_rows_kernel(const float* __restrict__ s, T* __restrict__ p, long long rows,
                                                           int n, float scale) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* sr = s + row * n;
    float mx = -INFINITY;
    for (int j = lane; j < n; j += 64) mx = fmaxf(mx, sr[j] * scale);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float sum = 0.f;
    for (int j = lane; j < n; j += 64) sum += expf(sr[j] * scale - mx);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
    const float inv = 1.0f / sum;
    for (int j = lane; j < n; j += 64) p[row * n + j] = Elem<T>::from_f32(expf(sr[j] * scale - mx) * inv);
}

// out[i] = T(x[i])   (raw copy of the fp32 stream as a GEMM operand: the 1x1 shortcut convolution)
template <typename T>
__global__ void cast_kernel(const float* __restrict__ x, T* __restrict__ out, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = Elem<T>::from_f32(x[i]);
}

inline dim3 grid1d(long long n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

hipError_t launch_vae_input(const float* z, const float* w, const float* b, float inv_scale, float* out, int B, int HW,
                            hipStream_t s) {
    hipLaunchKernelGGL(vae_input_kernel, grid1d((long long)B * HW), dim3(256), 0, s, z, w, b, inv_scale, out, B, HW);
    return hipGetLastError();
}
hipError_t launch_vae_output(const float* in, float* out, int B, int C, int HW, int ldc, hipStream_t s) {
    hipLaunchKernelGGL(vae_output_kernel, grid1d((long long)B * C * HW), dim3(256), 0, s, in, out, B, C, HW, ldc);
    return hipGetLastError();
}
template <typename T>
hipError_t launch_im2col3x3(const T* src, T* dst, int B, int H, int W, int C, int up, int Kpad, hipStream_t s) {
    constexpr int V = 16 / (int)sizeof(T);
    if (C % V || Kpad % V || Kpad < 9 * C) return hipErrorInvalidValue;
    const long long total = (long long)B * H * W * (Kpad / V);
    hipLaunchKernelGGL(im2col3x3_kernel<T>, grid1d(total), dim3(256), 0, s, src, dst, B, H, W, C, up, Kpad);
    return hipGetLastError();
}
template <typename T>
hipError_t launch_im2col3x3_s2(const T* src, T* dst, int B, int H, int W, int C, int Kpad, hipStream_t s) {
    constexpr int V = 16 / (int)sizeof(T);
    if (C % V || Kpad % V || Kpad < 9 * C || H < 1 || W < 1) return hipErrorInvalidValue;
    const long long total = (long long)B * H * W * (Kpad / V);
    hipLaunchKernelGGL(im2col3x3_s2_kernel<T>, grid1d(total), dim3(256), 0, s, src, dst, B, H, W, C, Kpad);
    return hipGetLastError();
}
hipError_t launch_vae_image(const float* x, float* out, int B, int HW, hipStream_t s) {
    hipLaunchKernelGGL(vae_image_kernel, grid1d((long long)B * HW), dim3(256), 0, s, x, out, B, HW);
    return hipGetLastError();
}
hipError_t launch_vae_moments(const float* h, const float* w, const float* b, const float* eps, float* moments, float* z, int B, int HW,
                              hipStream_t s) {
    hipLaunchKernelGGL(vae_moments_kernel, grid1d((long long)B * HW), dim3(256), 0, s, h, w, b, eps, moments, z, B, HW);
    return hipGetLastError();
}
hipError_t launch_vae_sample(const float* moments, const float* eps, float* z, int B, int HW, hipStream_t s) {
    hipLaunchKernelGGL(vae_sample_kernel, grid1d((long long)B * 4 * HW), dim3(256), 0, s, moments, eps, z, B, HW);
    return hipGetLastError();
}
template <typename T>
hipError_t launch_im2col3x3_c4(const float* src, T* dst, int B, int H, int W, int Kpad, hipStream_t s) {
    hipLaunchKernelGGL(im2col3x3_c4_kernel<T>, grid1d((long long)B * H * W * Kpad), dim3(256), 0, s, src, dst, B, H, W, Kpad);
    return hipGetLastError();
}
template <typename T>
hipError_t launch_groupnorm(const float* x, float* part, const float* gamma, const float* beta, T* out, int B, int HW, int C,
                            int swish, hipStream_t s) {
    if (C % 128 || C > 1024) return hipErrorInvalidValue;   // float4 columns: a multiple of 32, at most 256 per block
    const int chunks = (HW + kGnChunk - 1) / kGnChunk;
    hipLaunchKernelGGL(gn_stats_kernel, dim3(B * chunks), dim3(256), 0, s, x, part, HW, C, chunks);
    float* stat = part + (long long)B * chunks * 64;      // (mean, rstd) per (image, group) behind the partials
    hipLaunchKernelGGL(gn_finalize_kernel, dim3((B * 32 + 255) / 256), dim3(256), 0, s, x, part, stat, B * 32, chunks,
                       HW, C, (double)HW * (C / 32));
    const long long total4 = (long long)B * HW * (C / 4);
    hipLaunchKernelGGL(gn_apply_kernel<T>, grid1d(total4), dim3(256), 0, s, x, stat, gamma, beta, out, HW, C, swish, total4);
    return hipGetLastError();
}
int groupnorm_partials(int B, int HW) { return B * ((HW + kGnChunk - 1) / kGnChunk) * 32 * 2 + B * 64; }
template <typename T>
hipError_t launch_softmax_rows(const float* sc, T* p, long long rows, int n, float scale, hipStream_t s) {
    hipLaunchKernelGGL(softmax_rows_kernel<T>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, sc, p, rows, n, scale);
    return hipGetLastError();
}
template <typename T>
hipError_t launch_cast(const float* x, T* out, long long n, hipStream_t s) {
    hipLaunchKernelGGL(cast_kernel<T>, grid1d(n), dim3(256), 0, s, x, out, n);
    return hipGetLastError();
}

#define DD_INST(T)                                                                                                     \
    template hipError_t launch_im2col3x3<T>(const T*, T*, int, int, int, int, int, int, hipStream_t);                 \
    template hipError_t launch_im2col3x3_s2<T>(const T*, T*, int, int, int, int, int, hipStream_t);                   \
    template hipError_t launch_im2col3x3_c4<T>(const float*, T*, int, int, int, int, hipStream_t);                    \
    template hipError_t launch_groupnorm<T>(const float*, float*, const float*, const float*, T*, int, int, int, int, \
                                            hipStream_t);                                                             \
    template hipError_t launch_softmax_rows<T>(const float*, T*, long long, int, float, hipStream_t);                 \
    template hipError_t launch_cast<T>(const float*, T*, long long, hipStream_t);
DD_INST(bf16_t)
DD_INST(float)
#undef DD_INST

}  // namespace dd
