// Wave-level building blocks shared by the kernel translation units (gfx950 only): each exists ONCE, here.  Only what at least two
// kernels use lives in this header.  Changing one of them changes every kernel that calls it: the rule is that the gfx950 code object
// of every translation unit stays instruction-for-instruction identical unless the change is meant to alter it (DESIGN.md section 4.3;
// the comparison is written down in profiles/wave_prims/kernel_object_hashes.txt).
#pragma once
#include "dd_internal.h"

namespace dd {

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

// two floats -> one packed bf16 pair: one v_cvt_pk_bf16_f32 (round to nearest even, as f2bf)
__device__ __forceinline__ unsigned cvt_pk_bf16(float lo, float hi) {
    typedef __bf16 bf16v2 __attribute__((ext_vector_type(2)));
    typedef float f32v2 __attribute__((ext_vector_type(2)));
    const f32v2 q = {lo, hi};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(q, bf16v2));
}

// the 32-bit LDS address of a pointer into shared memory (what ds_* instructions and M0 take)
__device__ __forceinline__ unsigned lds_offset(const void* p) { return (unsigned)(size_t)(const __attribute__((address_space(3))) char*)p; }

// One 1 KB LDS-DMA piece (64 lanes x 16 bytes, lane-linear in LDS from lds_dst), per-lane source pointers: hipcc emits the M0 setup itself.
__device__ __forceinline__ void lds_dma16(const void* src, void* lds_dst) {
    __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)lds_dst, 16, 0, 0);
}
// The same piece in the scalar-base form: uniform 64-bit base (SGPRs) + a 32-bit lane offset, M0 = the piece's LDS address.  Written as asm: the builtin turns
// base + offset into a 64-bit VGPR address pair (checked in the ISA), and that form serialises with the SIMD's MFMAs (profiles/r05/dma_mfma_probe_roles.txt).
// s_nop 0: gfx950 needs one wait state between an SALU write of M0 and the request that reads it, and hipcc does not pad the inside of an asm string
// (without it the request may use the previous M0 and put its piece in another piece's slot; tools/isa_audit_lds_dma.py checks every request of every kernel).
__device__ __forceinline__ void lds_dma16s(const char* sbase, unsigned voff, const void* lds_dst) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(lds_offset(lds_dst)), "v"(voff), "s"(sbase) : "memory", "m0");
}

template <int N>
__device__ __forceinline__ void waitcnt_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"i"(N) : "memory"); }

// 16-byte LDS read at a compile-time offset from one address register, as asm: hipcc does not count it -- the reader waits (lgkmcnt) itself
template <int OFF, typename V>
__device__ __forceinline__ void ds_read16(V& dst, unsigned addr) {
    static_assert(sizeof(V) == 16, "one ds_read_b128");
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "i"(OFF));
}

// ONE gap of a hand-scheduled MFMA stream as ONE asm statement:
//     [s_waitcnt lgkmcnt(LG): at most LG LDS reads younger than this MFMA's fragment are outstanding; LG < 0: the gap in front already waited for it]
//     MFMA 32x32x16 bf16, acc += wa . xb   [READ: ds_read_b128 of the fragment some gaps ahead, into the register the MFMA just read]
// AGPR: the accumulator's register class (the AGPR half of the register file, or VGPRs where VALU code reads the tile).  Each form names only the operands it uses.
#define DD_S_MFMA_W "s_waitcnt lgkmcnt(%[lg])\n\tv_mfma_f32_32x32x16_bf16 %[acc], %[wa], %[xb], %[acc]"
#define DD_S_MFMA_N "v_mfma_f32_32x32x16_bf16 %[acc], %[wa], %[xb], %[acc]"
#define DD_S_READ "\n\tds_read_b128 %[wa], %[la] offset:%[lo]"
#define DD_MFMA_GAP(ACC_C)                                                                                                                                \
    if constexpr (LG >= 0) {                                                                                                                              \
        if constexpr (READ) asm volatile(DD_S_MFMA_W DD_S_READ : [acc] ACC_C(acc), [wa] "+v"(wa) : [xb] "v"(xb), [la] "v"(la), [lg] "i"(LG), [lo] "i"(LO)); \
        else asm volatile(DD_S_MFMA_W : [acc] ACC_C(acc), [wa] "+v"(wa) : [xb] "v"(xb), [lg] "i"(LG));                                                    \
    } else {                                                                                                                                              \
        if constexpr (READ) asm volatile(DD_S_MFMA_N DD_S_READ : [acc] ACC_C(acc), [wa] "+v"(wa) : [xb] "v"(xb), [la] "v"(la), [lo] "i"(LO));              \
        else asm volatile(DD_S_MFMA_N : [acc] ACC_C(acc), [wa] "+v"(wa) : [xb] "v"(xb));                                                                  \
    }
template <bool AGPR, int LG, bool READ, int LO>
__device__ __forceinline__ void mfma_gap(f32x16& acc, bf16x8& wa, const bf16x8& xb, unsigned la) {
    if constexpr (AGPR) { DD_MFMA_GAP("+a") } else { DD_MFMA_GAP("+v") }
}
#undef DD_MFMA_GAP

// 64-lane butterfly sum: every lane receives the total
__device__ __forceinline__ float wave_reduce_add(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Extra-token row idx (the B * tok_e time / label rows of a batch, image-major; clamped to the last one) -> its token row: image b's tokens are
// rows [b * tok_l, (b + 1) * tok_l), the extras first
__device__ __forceinline__ long long extra_token_row(int idx, int n_extra, int tok_e, int tok_l) {
    const int q = idx < n_extra ? idx : n_extra - 1, b = q / tok_e;
    return (long long)b * tok_l + (q - b * tok_e);
}

}  // namespace dd
