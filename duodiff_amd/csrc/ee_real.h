// Real early exit (ee_real.hip): the records its kernels and the host driver (loops.hip) share.  Host and device.
#pragma once
#include "dd_internal.h"

namespace dd {

constexpr int EE_REAL_MAX_SLOTS = 1024;        // images of one chain (the decision kernel keeps one flag per slot in LDS)
constexpr int EE_REAL_MAX_SLABS = 40;          // buffers one compaction moves: x, xfrag, one norm1 form, xb, and two per in-block
constexpr long long EE_REAL_PIECE = 65536;     // bytes of a slab one workgroup of the compaction copies

// one per-image buffer of a chain: image (slot) i occupies bytes [i * bytes, (i + 1) * bytes) behind base
struct RealSlab { char* base; long long bytes; };
struct RealSlabs { RealSlab s[EE_REAL_MAX_SLABS]; int n; };

// a chain's tables on the device: tab [B] slot -> image; rec [B] (exit layer or depth, slot) per image; counts [2] = (Ba', moves) of the
// last compaction layer; moves [B / 2 + 1] (source slot, destination slot)
struct RealTables { int* tab; int* rec; int* counts; int* moves; };

// the hole-fill plan on the host (the rule the decision kernel applies): alive [Ba] -> Ba', *n_moves and moves_src_dst [2 * n_moves]
int real_exit_plan(const int* alive, int Ba, int* n_moves, int* moves_src_dst);

hipError_t launch_ee_real_decide(const float* cls_l, float thr, int layer, int depth, int Ba, bool compact, const RealTables& t, int* idx_tab,
                                 int idx_stride, int idx_col0, const StepState* st, hipStream_t s);
hipError_t launch_ee_real_compact(const RealTables& t, int n_moves, const RealSlabs& slabs, hipStream_t s);
hipError_t launch_ee_real_step(float* x, const float* outs, const float* eps, const RealTables& t, float thr, int depth, StepState* st, const StepCoef* coef,
                               int B, int C, int S, int noise_mode, int b0, const unsigned long long* seeds, hipStream_t s);

}  // namespace dd
