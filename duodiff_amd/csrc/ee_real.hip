// Real early exit (dd_sample_early_exit_real): the kernels that let the early-exit loop stop running an image once it has left.
// The active images of a chain sit in the slots [0, Ba) of every per-image buffer; a slot -> image table says who sits where (the identity
// at the start of every step).  Behind layer l's probe one decision launch records who leaves; at a compaction layer it also plans the moves
// that close the holes, and a copy launch carries them out on every buffer that is live in front of block l.  The step kernel then reads
// each image's model output where its exit left it.  No kernel of the forward changes: a row takes the same kernel and the same bits in
// any slot of any batch, so every image gets the bits dd_sample_early_exit selects for it.
//
// Host-side restatement of: the exit rule of the reference's early-exit sampler (eesampler.py:61-82), applied while the forward runs.
#include "dd_internal.h"
#include "step_update.h"
#include "ee_real.h"

namespace dd {

// The hole-fill plan, defined once for the host (tests, the CPU restatement) and the device (the decision kernel's one planning thread):
// alive[s] != 0 for the slots [0, Ba) that still run.  Returns Ba' = their number; the holes among [0, Ba') in increasing order are filled
// by the surviving slots >= Ba' in increasing order: moves[k] = (src, dst).  Sources lie in [Ba', Ba), destinations in [0, Ba'): disjoint.
__host__ __device__ inline int real_exit_plan_impl(const int* alive, int Ba, int* n_moves, int2* moves) {
    int keep = 0;
    for (int s = 0; s < Ba; ++s) keep += alive[s] != 0;
    int n = 0, src = keep;
    for (int dst = 0; dst < keep; ++dst) {
        if (alive[dst]) continue;
        while (!alive[src]) ++src;       // (as many survivors sit at or behind `keep` as there are holes in front of it)
        moves[n++] = int2{src++, dst};
    }
    *n_moves = n;
    return keep;
}
int real_exit_plan(const int* alive, int Ba, int* n_moves, int* moves_src_dst) {
    return real_exit_plan_impl(alive, Ba, n_moves, (int2*)moves_src_dst);
}

namespace {

// One workgroup per (layer, chain), behind the layer's probe.  cls_l: the layer's row of the predicted errors, by slot.  For every active
// slot whose image has not left yet: it leaves here if cls <= thr.  rec[image] = (exit layer or depth, the slot the image sat in when that
// layer's head ran -- for an image still running: the slot it sits in now).  The idx table's entry is written at layer 0 and at the first
// exit; what layer 0 writes for an image that stays is ee_exit_layer's closing value: depth -- or 0 where thr is not >= 0 at all (no layer
// passes and the appended zero does not either: the reference's argmax of an all-False column; such an image still runs every block, since a
// later layer may pass, and ee_real_step_kernel hands it head 0's output).  compact: thread 0 then plans the moves, permutes the table and
// writes counts = (Ba', moves).
__global__ void __launch_bounds__(256) ee_real_decide_kernel(const float* __restrict__ cls_l, float thr, int layer, int depth, int Ba, int compact,
                                                             int* __restrict__ tab, int2* __restrict__ rec, int* __restrict__ counts,
                                                             int2* __restrict__ moves, int* __restrict__ idx_tab, int idx_stride, int idx_col0,
                                                             const StepState* __restrict__ st) {
    __shared__ int alive[EE_REAL_MAX_SLOTS];
    const int never = (0.0f <= thr) ? depth : 0;
    for (int s = threadIdx.x; s < Ba; s += 256) {
        const int img = layer == 0 ? s : tab[s];
        if (layer == 0) tab[s] = s;
        int2 r = layer == 0 ? int2{depth, s} : rec[img];
        const bool was_in = r.x == depth;
        if (was_in) {
            r.y = s;
            if (cls_l[s] <= thr) r.x = layer;
            rec[img] = r;
            if (idx_tab && (layer == 0 || r.x == layer)) idx_tab[(long long)st->t_final * idx_stride + idx_col0 + img] = r.x == depth ? never : r.x;
        }
        alive[s] = r.x == depth;
    }
    if (!compact) return;
    __syncthreads();
    if (threadIdx.x != 0) return;
    int n = 0;
    const int keep = real_exit_plan_impl(alive, Ba, &n, moves);
    for (int k = 0; k < n; ++k) {
        const int2 mv = moves[k];
        const int in = tab[mv.x], out = tab[mv.y];
        tab[mv.y] = in; tab[mv.x] = out;       // (the table stays a permutation: the image that left takes the vacated slot)
        rec[in].y = mv.y;
    }
    counts[0] = keep; counts[1] = n;
}

// blockIdx.x: the move, blockIdx.y: the buffer, blockIdx.z: a 64 KB piece of the slab.  16-byte accesses; a slab is a multiple of 16 bytes
// (the host asserts it) and source and destination slots differ, so the copy runs in place with no order between workgroups.
__global__ void __launch_bounds__(256) ee_real_compact_kernel(const int2* __restrict__ moves, RealSlabs slabs) {
    const int2 mv = moves[blockIdx.x];
    const RealSlab sl = slabs.s[blockIdx.y];
    const long long lo = (long long)blockIdx.z * EE_REAL_PIECE, hi = lo + EE_REAL_PIECE < sl.bytes ? lo + EE_REAL_PIECE : sl.bytes;
    const char* src = sl.base + (long long)mv.x * sl.bytes;
    char* dst = sl.base + (long long)mv.y * sl.bytes;
    for (long long o = lo + (long long)threadIdx.x * 16; o < hi; o += 256 * 16) *(u32x4*)(dst + o) = *(const u32x4*)(src + o);
}

// ee_select_step_kernel's sibling: image b's model output is head e's at the slot the image sat in when that head ran (outs [depth, B, C, S,
// S] by slot), or eps at its final slot where it never left -- head 0's at slot b (layer 0's table is the identity) where thr is not >= 0:
// ee_exit_layer's closing rule; the update, the draw (by IMAGE: b0 + b) and the advance are that kernel's.
__global__ void __launch_bounds__(256) ee_real_step_kernel(float* __restrict__ x, const float* __restrict__ outs, const float* __restrict__ eps,
                                                           const int2* __restrict__ rec, float thr, int depth, StepState* st,
                                                           const StepCoef* __restrict__ coef, int B, int C, int S, int noise_mode, int advance,
                                                           int b0, const unsigned long long* __restrict__ seeds) {
#pragma clang fp contract(off)
    const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long hw = (long long)S * S;
    const StepRule<false> rule(st, coef, nullptr, nullptr, noise_mode == 2 ? 2 : 0, 0, advance);
    if (pix == 0) rule.advance(st);
    if (pix >= (long long)B * hw) return;
    const long long b = pix / hw, p = pix - b * hw;
    f32x4 zn = {0.f, 0.f, 0.f, 0.f};
    if (rule.draws()) {
        const DrawSite ds = draw_site(seeds, st->seed, (unsigned long long)(b + b0), (unsigned long long)p, (unsigned long long)hw);
        zn = philox_normal4(ds.key, ds.id, rule.ctr);
    }
    int2 r = rec[b];
    if (r.x == depth && !(0.0f <= thr)) r = int2{0, (int)b};
    const float* src = (r.x == depth ? eps : outs + (long long)r.x * B * C * hw) + (long long)r.y * C * hw;
    for (int c = 0; c < C; ++c) {
        const long long e = (b * C + c) * hw + p;
        x[e] = rule.apply(x[e], src[c * hw + p], zn[c], 0.f);
    }
}

}  // namespace

hipError_t launch_ee_real_decide(const float* cls_l, float thr, int layer, int depth, int Ba, bool compact, const RealTables& t, int* idx_tab,
                                 int idx_stride, int idx_col0, const StepState* st, hipStream_t s) {
    if (Ba < 1 || Ba > EE_REAL_MAX_SLOTS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ee_real_decide_kernel, dim3(1), dim3(256), 0, s, cls_l, thr, layer, depth, Ba, compact ? 1 : 0, t.tab, (int2*)t.rec, t.counts,
                       (int2*)t.moves, idx_tab, idx_stride, idx_col0, st);
    return hipGetLastError();
}

hipError_t launch_ee_real_compact(const RealTables& t, int n_moves, const RealSlabs& slabs, hipStream_t s) {
    if (n_moves < 1 || slabs.n < 1 || slabs.n > EE_REAL_MAX_SLABS) return hipErrorInvalidValue;
    long long most = 0;
    for (int i = 0; i < slabs.n; ++i) {
        if (slabs.s[i].bytes < 16 || slabs.s[i].bytes % 16 || (uintptr_t)slabs.s[i].base % 16) return hipErrorInvalidValue;
        most = slabs.s[i].bytes > most ? slabs.s[i].bytes : most;
    }
    const dim3 grid((unsigned)n_moves, (unsigned)slabs.n, (unsigned)((most + EE_REAL_PIECE - 1) / EE_REAL_PIECE));
    hipLaunchKernelGGL(ee_real_compact_kernel, grid, dim3(256), 0, s, (const int2*)t.moves, slabs);
    return hipGetLastError();
}

hipError_t launch_ee_real_step(float* x, const float* outs, const float* eps, const RealTables& t, float thr, int depth, StepState* st, const StepCoef* coef,
                               int B, int C, int S, int noise_mode, int b0, const unsigned long long* seeds, hipStream_t s) {
    const long long npix = (long long)B * S * S;
    hipLaunchKernelGGL(ee_real_step_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, x, outs, eps, (const int2*)t.rec, thr, depth, st, coef, B, C,
                       S, noise_mode, 1, b0, seeds);
    return hipGetLastError();
}

}  // namespace dd
