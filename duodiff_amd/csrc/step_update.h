// The sampling-step update, defined once (device only).  Loops, chains, cut loops and manual steps are compared bit for bit, so the
// operation order and the roundings below are a contract: every step kernel (step.hip) applies these functions and holds no update
// arithmetic of its own.  Each function that rounds carries the fp-contract pragma in its own body (at file scope it would leak into the
// including unit): mul, sub, mul, add -- no FMA, as the reference rounds.
#pragma once
#include "dd_internal.h"

namespace dd {

// ------------------------------------------------------------------------------------------
// Device noise: Philox4x32-10 counter RNG + Box-Muller.  Counter = (element/4, t, 0, 0),
// key = seed.  Statistically N(0,1); NOT the torch CPU mt19937 stream (that is DD_NOISE_BUFFER).
// The fourth counter word names the stream: PHILOX_STEP for the update's z, PHILOX_KNOWN for the z2 of a known region --
// the same key, pixel and counter give two independent draws.  PHILOX_START is the stream of x_T (dd_noise_images).
// ------------------------------------------------------------------------------------------
constexpr unsigned PHILOX_STEP = 0x5eedu, PHILOX_KNOWN = 0x6b6e6f77u, PHILOX_START = 0x78545f30u;
constexpr unsigned PHILOX_SCAN = 0x7363616e;      // "scan": the z that noises a real image in the denoising-error scan (scan_target below)
constexpr unsigned PHILOX_JUMP = 0x6a756d70;      // "jump": the z3 of a resampling jump (jump below); z, z2 and z3 of one counter are three independent draws

// The draw site, defined once: the Philox key and pixel id of pixel p = y S + x (hw = S S pixels per image) of image bg of the WHOLE batch
// (bg = the launch's first image b0 + the launch's image b: a half-batch chain draws what the undivided batch would).
//   plain  (seeds == null)  key = seed,       id = bg hw + p    -- the batch-wide pixel id: an image's noise depends on where it sits
//   seeded                  key = seeds[bg],  id = p            -- per-image seeds (dd_set_image_seeds): it depends on its seed alone
// so a seeded image with seed s draws exactly what the plain call with B = 1 and seed = s draws.  `seeds` is a launch argument: the
// branch is uniform.  Every drawing kernel takes (key, id) from here and holds no id arithmetic of its own.
struct DrawSite { unsigned long long key, id; };
__device__ __forceinline__ DrawSite draw_site(const unsigned long long* __restrict__ seeds, unsigned long long seed, unsigned long long bg,
                                              unsigned long long p, unsigned long long hw) {
    if (seeds) return DrawSite{seeds[bg], p};
    return DrawSite{seed, bg * hw + p};
}
__device__ __forceinline__ void philox_round(unsigned& c0, unsigned& c1, unsigned& c2, unsigned& c3,
                                             unsigned k0, unsigned k1) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
}

// four N(0,1) values for one pixel (one per channel, C <= 4): counter = (pixel, t), key = seed
__device__ __forceinline__ f32x4 philox_normal4(unsigned long long seed, unsigned long long pixel, int t, unsigned stream = PHILOX_STEP) {
    unsigned c0 = (unsigned)pixel, c1 = (unsigned)(pixel >> 32), c2 = (unsigned)t, c3 = stream;
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c0, c1, c2, c3, k0, k1);
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    // Box-Muller on (c0,c1) and (c2,c3); hardware log/sin/cos (|error| ~1e-6) are ample for noise
    const float ua = ((float)c0 + 1.0f) * 2.3283064365386963e-10f, ub = (float)c1 * 2.3283064365386963e-10f;
    const float uc = ((float)c2 + 1.0f) * 2.3283064365386963e-10f, ud = (float)c3 * 2.3283064365386963e-10f;
    const float ra = sqrtf(-2.0f * __logf(ua)), rc = sqrtf(-2.0f * __logf(uc));
    const float aa = 6.283185307179586f * ub, ac = 6.283185307179586f * ud;
    return f32x4{ra * __cosf(aa), ra * __sinf(aa), rc * __cosf(ac), rc * __sinf(ac)};
}

// One step's rule, built once per thread:
//   DDPM   x' = c1 (x - c2 eps) + sigma z                      (reference sampler.py:47-56)
//   table  x' = a x + b eps [+ d h if hist] [+ c z if drawn],  h' = p x + q eps   (AffineRow / HistRow of step k)
// H: the rule carries a history part (the multistep loop); H = false compiles to the code without it.
// noise_mode: 0 none, 1 a z buffer the caller reads where reads_z(), 2 Philox where draws() with counter ctr.
template <bool H>
struct StepRule {
    int t;                        // st->t_final as read: the timestep (DDPM) or the step index (table)
    bool table, draw;             // draw: this step adds noise at all (t > 0, or row.noise)
    int noise_mode, ctr;
    StepCoef cf;
    float sigma;
    AffineRow row;
    HistRow hr;
    bool adv;
    float t_next;                 // table && adv: the next row's t_model

    // From the device-resident step state.  Every load is issued here, so a kernel builds the rule ahead of its own long-latency work;
    // none waits for another beyond the step state -> row chain (the caller likewise requests h without waiting for hr.hist).
    __device__ __forceinline__ StepRule(const StepState* st, const StepCoef* coef, const AffineRow* atab, const HistRow* htab,
                                        int noise_mode_, int variance, int advance)
        : t(st->t_final), table(atab != nullptr), noise_mode(noise_mode_), hr{0.f, 0.f, 0.f, 0}, adv(advance != 0) {
        row = table ? atab[t] : AffineRow{0.f, 0.f, 0.f, 0.f, 0, 0, 0, 0};
        t_next = (table && adv) ? atab[t + 1].t_model : 0.f;
        cf = coef[table ? 0 : (t < 0 ? 0 : (t > 999 ? 999 : t))];
        draw = table ? (row.noise != 0) : (t > 0);
        if constexpr (H) hr = htab[t];
        ctr = table ? row.ctr : t;
        sigma = variance == 1 ? cf.sigma_beta : cf.sigma_tilde;
    }
    // From plain coefficients (the unfused step kernels): the same rule, nothing loaded and no step state to advance.
    __device__ __forceinline__ StepRule(StepCoef c, bool variance_beta, bool use_z)      // DDPM
        : t(0), table(false), draw(use_z), noise_mode(1), ctr(0), cf(c), sigma(variance_beta ? c.sigma_beta : c.sigma_tilde),
          row{0.f, 0.f, 0.f, 0.f, 0, 0, 0, 0}, hr{0.f, 0.f, 0.f, 0}, adv(false), t_next(0.f) {}
    __device__ __forceinline__ StepRule(float a, float b, float c, HistRow h, bool use_z)   // table row
        : t(0), table(true), draw(use_z), noise_mode(1), ctr(0), cf{0.f, 0.f, 0.f, 0.f}, sigma(0.f),
          row{0.f, a, b, c, use_z, 0, 0, 0}, hr(h), adv(false), t_next(0.f) {}

    __device__ __forceinline__ bool reads_z() const { return draw && noise_mode == 1; }
    __device__ __forceinline__ bool draws() const { return draw && noise_mode == 2; }
    __device__ __forceinline__ bool noisy() const { return reads_z() || draws(); }

    // x' from x, the model output, this element's z (read only where reads_z() / draws()) and its history h (read only where hr.hist:
    // a step without history never lets h into x' -- the first step's h may be an uninitialised buffer, and 0 * NaN is NaN)
    __device__ __forceinline__ float apply(float x, float eps, float z, float h) const {
#pragma clang fp contract(off)
        float v;
        if (table) {
            v = row.a * x + row.b * eps;
            if constexpr (H) {
                if (hr.hist) v = v + hr.d * h;
            }
            if (noisy()) v = v + row.c * z;
        } else {
            v = cf.c1 * (x - cf.c2 * eps);
            if (noisy()) v = v + sigma * z;
        }
        return v;
    }
    // h' of the multistep row, written on every step
    __device__ __forceinline__ float history(float x, float eps) const {
#pragma clang fp contract(off)
        return hr.p * x + hr.q * eps;
    }
    // hands the next step its t / t_model; ONE thread of the step's last kernel calls it (no block of that kernel reads t / t_model)
    __device__ __forceinline__ void advance(StepState* st) const {
        if (!adv) return;
        const int tn = table ? t + 1 : t - 1;
        st->t = tn;
        st->t_model = table ? t_next : (float)tn;
    }
};

// The known region of a step (inpainting, the RePaint replacement rule without resampling): after the step has produced x', a pixel
// with mask m is finished from the known image x0 re-noised to the level the step lands on,
//     kn = ka x0 [+ kb z2  if kb != 0 and a z2 is there]        x'' = x' if m == 0, else m kn + (1 - m) x'
// each product rounded on its own, in that order.  m == 0 keeps x' bit for bit whatever x0 holds; m == 1 with finite x' gives kn
// (kn + 0: the value, a -0 becoming +0).  h' of the multistep rule is none of its business.
__device__ __forceinline__ float known(float xp, float x0, float m, float ka, float kb, float z2, bool use_z2) {
#pragma clang fp contract(off)
    if (m == 0.f) return xp;
    float kn = ka * x0;
    if (use_z2 && kb != 0.f) kn = kn + kb * z2;
    return m * kn + (1.f - m) * xp;
}
// known() in two halves, for a kernel that has x0 and z2 long before x' (threshold_step_kernel holds one register per element instead
// of two): known(xp, x0, m, ...) == known_mix(xp, known_value(x0, ...), m), the same products and sums in the same order
__device__ __forceinline__ float known_value(float x0, float ka, float kb, float z2, bool use_z2) {
#pragma clang fp contract(off)
    float kn = ka * x0;
    if (use_z2 && kb != 0.f) kn = kn + kb * z2;
    return kn;
}
__device__ __forceinline__ float known_mix(float xp, float kn, float m) {
#pragma clang fp contract(off)
    if (m == 0.f) return xp;
    return m * kn + (1.f - m) * xp;
}
// row t of a loop's known-region table (t as StepRule reads it: the timestep of the DDPM loop, the step index of a table-driven one),
// loaded behind the step state like the rule's own row
struct KnownRule {
    KnownRow row;
    bool philox;
    __device__ __forceinline__ KnownRule(const KnownRow* ktab, bool table, int t, int noise_mode)
        : row(ktab ? ktab[table ? t : (t < 0 ? 0 : (t > 999 ? 999 : t))] : KnownRow{0.f, 0.f}), philox(noise_mode == 2) {}   // (null: no known region)
    __device__ __forceinline__ bool draws() const { return philox && row.kb != 0.f; }
    __device__ __forceinline__ float apply(float xp, float x0, float m, float z2) const { return known(xp, x0, m, row.ka, row.kb, z2, philox); }
    __device__ __forceinline__ float value(float x0, float z2) const { return known_value(x0, row.ka, row.kb, z2, philox); }
};

// A resampling jump (RePaint's resampling, Restart sampling: dd_sample_affine_walk, dd_jump_step): x at the noise level of timestep s goes
// back up to that of timestep u >= s by forward noising, with no model evaluation,
//     x' = ja x [+ jc z3  if a z3 is there]        ja = sqrt(abar[u] / abar[s]), jc = sqrt(1 - abar[u] / abar[s])
// each product rounded on its own.  Every pixel takes it, the known ones of a region too: they are at level s and land at level u.
__device__ __forceinline__ float jump(float x, float z3, float ja, float jc, bool use_z3) {
#pragma clang fp contract(off)
    const float v = ja * x;
    return use_z3 ? v + jc * z3 : v;
}

// The denoising-error scan (dd_scan_error; reference trainer.py:307-352 evaluated at one timestep): an image x0 is noised to row k's level
// with a z of its own stream word, x_t = known_value(x0, ka, kb, z, true) = ka x0 + kb z, the model sees x_t, and its output m is compared with
//     tgt = tz z + t0 x0 + tx x_t      predict_noise (1, 0, 0) | predict_original (0, 1, 0) | predict_previous (0, clean_image_coef, noisy_image_coef)
//     err = (1 / CHW) sum (m - tgt)^2
// each product, sum and square rounded on its own, the sum taken left to right.  The reduction order belongs to the kernel (scan.hip).
__device__ __forceinline__ float scan_target(float z, float x0, float xt, float tz, float t0, float tx) {
#pragma clang fp contract(off)
    return tz * z + t0 * x0 + tx * xt;
}
// one element's share of the sum: acc + (m - tgt)^2
__device__ __forceinline__ float scan_accumulate(float acc, float m, float tgt) {
#pragma clang fp contract(off)
    const float d = m - tgt;
    return acc + d * d;
}
// the mean over an image's n = C H W elements (n <= 2^24: exact as a float), a correctly rounded division
__device__ __forceinline__ float scan_mean(float sum, int n) { return __fdiv_rn(sum, (float)n); }

// tanh|d| for the early-exit scan's second loss (dd_scan_error_early_exit; reference trainer.py:376, u_t_hats = mean(tanh|ee_output - true_output|)):
// the probes' training target.  No library tanhf / expf: only individually rounded + and x, two correctly rounded divisions, fabs and min, so
// that a numpy-float32 mirror (duodiff_amd/threshold_scan.py tanh_abs_f32) reproduces it bit for bit.  With a = min(|d|, 10), h = a / 2, s = h h:
//     t = h (135135 + 17325 s + 378 s^2 + s^3) / (135135 + 62370 s + 3150 s^2 + 28 s^3)     Lambert's continued fraction of tanh h, 7 levels
//     tanh a = min(2 t / (1 + t t), 1)                                                       the double-argument formula
// an odd rational in |d| behind a clamp; every coefficient is an integer, exact in fp32, and every term is >= 0 (no cancellation).  The result
// lies in [0, 1] and scan_tanh_abs(0) == 0.  inf gives the clamp's value; a NaN is not an argument (fminf drops it).
// E_TANH: the largest |scan_tanh_abs(d) - tanh|d|| over EVERY fp32 d against float64 tanh, swept on the CPU with the mirror
// (tools/scan_tanh_sweep.py: all 1 092 616 193 values of [0, 10] and the clamp's tail) = 1.66e-7
// (1.6533e-7, taken at d = 1.1165210; spec: <= 1e-6); the tests' bounds take it from tests/scan_support.py E_TANH.
constexpr float SCAN_TANH_CLAMP = 10.f;
__device__ __forceinline__ float scan_tanh_abs(float d) {
#pragma clang fp contract(off)
    const float h = 0.5f * fminf(fabsf(d), SCAN_TANH_CLAMP);
    const float s = h * h;
    const float p = ((s + 378.f) * s + 17325.f) * s + 135135.f;
    const float q = ((28.f * s + 3150.f) * s + 62370.f) * s + 135135.f;
    const float t = __fdiv_rn(h * p, q);
    return fminf(__fdiv_rn(t + t, t * t + 1.f), 1.f);
}
// one element's share of the second sum: acc + tanh|m - tgt|
__device__ __forceinline__ float scan_accumulate_tanh(float acc, float m, float tgt) {
#pragma clang fp contract(off)
    const float d = m - tgt;
    return acc + scan_tanh_abs(d);
}

// x0 thresholding of a multistep step (dd_x0_threshold): the step's data prediction x0 = p x + q m (StepRule::history) is pulled back
// before it drives the update, and the update then takes it in m's place -- a and b are the UNFOLDED row, b multiplying xh:
//     static   xh = min(max(x0, -r), r)
//     dynamic  s  = v[i] + f (v[i1] - v[i]),  v = |x0| of ONE image ascending (sub, mul, add);  s = min(max(s, 1), smax)
//              xh = min(max(x0, -s), s) / s          (correctly rounded division)
//     x' = StepRule<true>::apply(x, xh, z, h)        h' = xh
// v[i], v[i1] come from an exact selection on the bit patterns of |x0| (threshold_step_kernel), never from an approximation; i and f
// from the host (dd_internal.h X0Threshold).
__device__ __forceinline__ float threshold_scale(float vi, float vi1, float f, float s_max) {
#pragma clang fp contract(off)
    const float s = vi + f * (vi1 - vi);
    return fminf(fmaxf(s, 1.f), s_max);
}
__device__ __forceinline__ float threshold_clip(float x0, float s, bool divide) {
    const float v = fminf(fmaxf(x0, -s), s);
    return divide ? __fdiv_rn(v, s) : v;
}

// eesampler.py:61-67: idx[b] = first layer i in [0, depth] with c[i][b] <= threshold, where c[depth][b] = 0 closes the
// list (torch.argmax of an all-False column is 0)
__device__ __forceinline__ int ee_exit_layer(const float* __restrict__ cls, float thr, int depth, int B, int b) {
    int idx = -1;
    for (int k = 0; k < depth && idx < 0; ++k)
        if (cls[(long long)k * B + b] <= thr) idx = k;
    if (idx < 0) idx = (0.0f <= thr) ? depth : 0;
    return idx;
}

}  // namespace dd
