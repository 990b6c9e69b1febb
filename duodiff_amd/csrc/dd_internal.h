// Internal declarations shared by the HIP translation units of libduodiff.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernel_table.h"

namespace dd {

typedef unsigned short bf16_t;  // raw bf16 bits

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bf16_t f2bf(float f) {
    __bf16 b = (__bf16)f;  // v_cvt_pk_bf16_f32: round-to-nearest-even, NaN stays NaN
    return __builtin_bit_cast(unsigned short, b);
}
__device__ __forceinline__ float bf2f(bf16_t b) {
    return __builtin_bit_cast(float, ((unsigned)b) << 16);
}

template <typename T> struct Elem;
template <> struct Elem<float> {
    static constexpr int kPerChunk = 4;  // elements per 16-byte chunk
    __device__ static __forceinline__ float from_f32(float v) { return v; }
    __device__ static __forceinline__ float to_f32(float v) { return v; }
};
template <> struct Elem<bf16_t> {
    static constexpr int kPerChunk = 8;
    __device__ static __forceinline__ bf16_t from_f32(float v) { return f2bf(v); }
    __device__ static __forceinline__ float to_f32(bf16_t v) { return bf2f(v); }
};

// Device-resident per-step state, so that a captured hipGraph replays without parameter
// patching: kernels read t from here, the last node of a step decrements it.
struct StepState {
    int t;            // current timestep (999 .. 0): read by the FIRST kernel of a step (token assembly) only
    float t_model;    // what the model sees: t or t/1000 is derived in the embed kernel
    unsigned long long seed;
    int t_final;      // copy of t made by the embed kernel and read by the LAST kernel of the step, which may then
                      // decrement t / t_model for the next replay without racing its own blocks (no separate launch)
    int pad;
};

// per-timestep update coefficients, x' = c1 (x - c2 eps) + sigma z
struct StepCoef {
    float c1, c2, sigma_tilde, sigma_beta;
};

// one step of a table-driven loop (dd_sample_affine): x' = a x + b eps + c z, the model sees t_model
struct AffineRow {
    float t_model, a, b, c;
    int noise, ctr, pad1, pad2;   // ctr: the Philox counter of this step's z (the step's index in the WHOLE loop, not in this call's table)
};
// dd_sample_multistep: the history part of step k's row, beside AffineRow k: x' = a x + b m [+ d h if hist] [+ c z], h' = p x + q m
struct HistRow {
    float d, p, q;
    int hist;                     // 0: h does not enter the update at all (0 * NaN is NaN: the first step, a caller's uninitialised buffer)
};

// the known-region half of step k's row (dd_known_region): the known pixels land on ka x0 + kb z2
struct KnownRow {
    float ka, kb;
};

// one step of the denoising-error scan (dd_scan_error; step_update.h scan_target): the images are noised to x_t = ka x0 + kb z, the model
// sees t_model, its output is compared with tz z + t0 x0 + tx x_t
struct ScanRow {
    float t_model, ka, kb, tz, t0, tx;
    int ctr, next;                // ctr: the Philox counter of this step's z (counter_base + the step's index in the call); next: the row the
                                  // early-exit scan hands on to (its table is indexed by timestep); dd_scan_error writes 0 and never reads it
};

enum GemmEpilogue {
    EPI_STORE = 0,        // out = T(acc)                                  (qkv)
    EPI_BIAS_GELU = 1,    // out = T(gelu_erf(acc + bias))                 (fc1)
    EPI_BIAS_RESID = 2,   // x += acc + bias ; optional out = T(x)         (proj, fc2)
    EPI_BIAS_SET = 3,     // x  = acc + bias                               (skip_linear)
    EPI_BIAS_STORE = 4,   // out = T(acc + bias)                           (VAE attention q/k projections)
    EPI_PARTIAL = 5       // partial[split] = acc over the split's k range (launch_gemm_splitk; launch_reduce_ln finishes the Linear)
};

// Head-major output map of the qkv Linear (what attention.hip reads): element (row m = b * L + l, column c) of the [M, 3D]
// result lives at ((b * 3H + (c >> 6)) * Lp + l) * 64 + (c & 63) -- the 64 columns of one (q | k | v, head) unit of one image
// are Lp contiguous 128-byte (bf16) rows, so a GEMM wave stores whole 4 KB blocks and the attention workgroup stages its K / V
// with linear LDS-DMA.  Lp = L rounded up to 8 (one LDS-DMA piece = 8 rows); rows l >= L are never written (the workspace
// is zeroed once).  L == 0: plain [M, ldo] rows.
struct HeadMajor {
    int L, Lp, H;
    unsigned magic;     // 2^32 / L + 1:  b = umulhi(m, magic)  (exact for m * L < 2^32)
};
inline HeadMajor make_head_major(int L, int H) {
    return HeadMajor{L, (L + 7) / 8 * 8, H, (unsigned)((1ull << 32) / (unsigned)L + 1ull)};
}
__device__ __forceinline__ long long hm_offset(const HeadMajor& hm, int row, int col) {
    const int b = (int)__umulhi((unsigned)row, hm.magic), l = row - b * hm.L;
    return (((long long)b * (3 * hm.H) + (col >> 6)) * hm.Lp + l) * 64 + (col & 63);
}

// C[M,N] = [A | A2][M,K] . W[N,K]^T ; A holds k < K1, A2 holds the rest (concat-free skip GEMM).
template <typename T>
struct GemmArgs {
    const T* A;
    const T* A2;
    const T* W;        // [N, K] row-major (nn.Linear layout)
    const float* bias; // [N] or null
    float* xres;       // fp32 [Mp, N] residual stream (EPI_BIAS_RESID / EPI_BIAS_SET)
    T* out;            // [Mp, ldo] or null
    int M, N, K, K1;
    int lda, lda2, ldo;
    HeadMajor hm;      // hm.L != 0: `out` is written head-major (the qkv Linear); N % 64 == 0
    float* partial = nullptr;   // launch_gemm_splitk: fp32 slabs [splits][M][N]
    int splits = 0;
    int tile128 = -1;           // bf16 launch_gemm: 1 = the 128 x 128 kernel, 0 = the 256 x 256 kernel where the shape fits it, -1 = decided from THIS call's shape
                                // (gemm_prefers_128).  The model's launches pass the decision made for its max_batch, so that a row's kernel never
                                // depends on the batch of a call (the two half-batch chains of dd_sample must compute what the whole batch computes)
};

// num_cus: CU count the persistent bf16 grid is sized for (per context; a multiple of 8)
template <typename T> hipError_t launch_gemm(const GemmArgs<T>& a, int epilogue, hipStream_t s, int num_cus);
bool plan_rows_256(int M, int N, int K, int num_cus, int* q, int* e);
bool gemm_prefers_128(int M, int N, int K, int K1, int num_cus);   // the 256 x 256 tiles of this shape would leave half of the CUs without one
bool gemm_splitk_supported(int M, int N, int K, int K1, int splits);
hipError_t launch_gemm_splitk(const GemmArgs<bf16_t>& a, hipStream_t s, int num_cus);
int device_num_cus();

// ---- fused MLP (mlp_fused.hip): x += fc2(gelu(fc1(h) + b1)) + b2 in one launch
struct MlpFusedArgs {
    const bf16_t* X;       // [Mp, ldx] LayerNorm output h (bf16); unused when ln_in_g is set
    int ldx;
    const float* ln_in_g;  // set: the kernel computes LayerNorm(x) * ln_in_g + ln_in_b itself from the residual rows
    const float* ln_in_b;  //      (the W1 image must then be packed with kperm = true)
    const bf16_t* ao;      // nproj > 0: attention output rows [Mp, D]; the kernel adds ao . Wproj^T + bproj to x first
    const float* bproj;    //            (main tiles only: the extra-token rows must already hold x1)
    int nproj;             // D / 32 blocks of Wproj in front of the MLP blocks of wimg, or 0
    const bf16_t* skip;    // nskip > 0: the NEXT block's skip_linear runs behind the MLP (main tiles): x' = [y | skip] . Wskip^T + bskip
    const float* bskip;    //            replaces y in xres, ln_out = norm1(x'); skip = the long-skip operand's rows [Mp, D]
    int nskip;             // 2 * D / 32 blocks of Wskip behind the MLP blocks of wimg (mlp_fused_pack_skip), or 0
    bf16_t* qkv_out;       // nqkv > 0: the NEXT block's attn.qkv (no bias) runs last (main tiles): qkv = norm1(updated rows) . Wqkv^T, written
    bf16_t* ln_out_frag;   // or null: the main tiles write norm1 HERE instead of ln_out, in MFMA fragment order ([32-row group of patch rows]
                           //          [D / 16 k-steps][64 lanes] x 16 bytes) for launch_qkv_attention; needs tok_n % 32 == 0
    bf16_t* qkv_dump;      //           head-major (hm) -- norm1 is then NOT written for the main rows; qkv_dump: 16 KB scratch (qkv | x | bf16 copy of rows past the end)
    HeadMajor hm;          //           (stores of rows past the end of a ragged tile)
    int nqkv;              // 3 * D / 32 blocks of Wqkv closing the image (mlp_fused_pack_rows), or 0
    const float* ln_out_g; // with ln_out: LayerNorm of the UPDATED rows, written as bf16 [Mp, D] (next block's norm1)
    const float* ln_out_b;
    bf16_t* ln_out;
    const char* wimg;      // weight image in MFMA fragment order (mlp_fused_pack)
    const float* b1p;      // fc1 bias, permuted to accumulator-register order per chunk
    const float* b2;       // [D]
    float* xres;           // fp32 [Mp, D] residual stream, updated in place
    bf16_t* out;           // optional bf16 copy of the updated rows, row stride ldo
    int ldo;
    float* partial;        // partial slabs of the hidden-split leftover tiles
    int nchunks;           // hidden / 32
    // row plan (mlp_fused_plan): token row of image b, token l = b * tok_l + l; tokens [0, tok_e) are the extras, then tok_n patches
    int tok_n, tok_e, tok_l;
    int n_main, n_extra;   // B * tok_n patch rows (main tiles), B * tok_e extra rows (hidden-split tiles)
    int tiles_main, tiles_left, groups, cpg;
    int prows;             // rows per hidden-split tile (32, 64 or 128: whole waves)
    float* y_tap = nullptr; // SKIP launches of early-exit models: the block output y (fp32 [Mp, D]) is stored here before skip_linear replaces it in xres -- the
                           // patch rows by the main tiles, the extra-token rows by the reduce launch (the next block's output head and probe read y)
    int reduce_set = 0;    // launch_mlp_reduce: x = b2 + slabs instead of x += (the extra-token rows of a row-resident skip_linear; of a block tail with the
                           // projection in front: the first hidden group's slab carries x + proj(ao) + b)
    const bf16_t* ao_frag = nullptr;   // nproj > 0, or null: the main tiles read the attention output of the PATCH rows here instead of ao, in MFMA fragment
                           // order ([32-row group of patch rows][D / 16 k-steps][64 lanes] x 16 bytes, natural k order: launch_qkv_attention's out_frag);
                           // the extra-token rows still come from ao; needs tok_n % 32 == 0
    bf16_t* out_frag = nullptr;        // or null (launches without skip phases): the main tiles write the bf16 copy of the PATCH rows here instead of out, in
                           // the same fragment order (k-step ks = columns 16 ks .. 16 ks + 15); the reduce launch still writes the extra-token rows to out
    const bf16_t* skip_frag = nullptr; // nskip > 0, or null: the SKIP phases read the long-skip operand's PATCH rows here (an in-block's out_frag) instead of
                           // skip; the extra-token rows (launch_skip_rows_ln) still come from skip
    const float* x_in_frag = nullptr;  // or null: the main tiles read the fp32 residual PATCH rows here instead of xres, as the previous tail left them:
                           // [32-row group][D / 32 tiles t][4 quads g][64 lanes] x 16 bytes, lane (r, h) of (t, g) = columns 32 t + 8 g + 4 h .. + 3 of row r
    float* x_out_frag = nullptr;       // or null: ... and write the updated rows here instead of xres, in that order.  Extra-token rows: always xres.
                           // The five hand-offs above: D = 512 with the projection in front, no qkv phases; x_*_frag not together with y_tap
};
// One 1 KB MFMA operand fragment of a row-major weight W (row stride ld): 64 lanes x 8 bf16 of the 32-row x 16-k piece at (row0, k0), lane = (row
// lane & 31, half h = lane >> 5) -- what one ds_read_b128 / 16-byte load per lane puts in front of a v_mfma_f32_32x32x16_bf16.  Element j of half h holds
// k0 + k(h, j), in one of two k orders: natural (the other operand is rows as loaded: 8 consecutive k per lane) or accumulator order (the other operand
// is converted from 32x32 accumulator registers: quads 2 kq, 2 kq + 1 of a tile, columns 8 g + 4 h .. + 3 each).  Every weight image of the library
// (mlp_fused_pack*, rowlin_pack, qkv_attention_pack) is a sequence of these.
enum FragK { FRAG_K_NATURAL = 0, FRAG_K_ACC = 1 };
__host__ __device__ constexpr int frag_k_natural(int h, int j) { return 8 * h + j; }
__host__ __device__ constexpr int frag_k_acc(int h, int j) { return 8 * (j >> 2) + 4 * h + (j & 3); }
inline void pack_fragment(const float* w, size_t ld, int row0, int k0, FragK order, unsigned short (*to_bf16)(float), unsigned short* dst) {
    for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 8; ++j) {
            const int h = lane >> 5, k = order == FRAG_K_ACC ? frag_k_acc(h, j) : frag_k_natural(h, j);
            dst[lane * 8 + j] = to_bf16(w[(size_t)(row0 + (lane & 31)) * ld + k0 + k]);
        }
}

// Layout of the fused block tail's weight image: blocks of D / 16 fragments (one ring slot of the kernel), four sections in stream order
//     [attn.proj: nproj blocks][fc1 / fc2 chunk pairs: 2 nchunks][next skip_linear: nskip][next attn.qkv: nqkv] + four run-off blocks
// (the kernel's DMA runs up to three blocks past the last one -- branch-free pipeline; never used as data).  The projection's section starts the image.
struct MlpImage {
    size_t blk;               // bytes per block
    size_t mlp, skip, qkv;    // first block of the section
    size_t end;               // blocks of data
    __host__ __device__ constexpr MlpImage(int D, int nproj, int nchunks, int nskip, int nqkv)
        : blk((size_t)(D / 16) * 1024), mlp((size_t)nproj), skip(mlp + 2 * (size_t)nchunks), qkv(skip + (size_t)nskip), end(qkv + (size_t)nqkv) {}
    static MlpImage of(int D, int hidden, bool with_proj, bool with_skip, bool with_qkv) {
        return MlpImage(D, with_proj ? D / 32 : 0, hidden / 32, with_skip ? D / 16 : 0, with_qkv ? 3 * D / 32 : 0);
    }
    __host__ __device__ constexpr size_t at(size_t block) const { return block * blk; }     // byte offset of a block
    constexpr size_t bytes() const { return at(end + 4); }
};
bool mlp_fused_supported(int D, int hidden);
// nn.Linear weight [nrows, D] -> nrows / 32 blocks (one 32-row tile each, fragment f = k-step f, k index in accumulator order)
void mlp_fused_pack_rows(int D, int nrows, const float* w, unsigned short (*to_bf16)(float), unsigned short* img);
// qkv of the extra-token rows of a QKV launch (from a.ln_out, which the reduce / skip_rows launch has written for them)
hipError_t launch_qkv_rows(const MlpFusedArgs& a, int D, hipStream_t s);
void mlp_fused_pack_proj(int D, const float* wp, unsigned short (*to_bf16)(float), unsigned short* img);
void mlp_fused_pack_skip(int D, const float* ws, unsigned short (*to_bf16)(float), unsigned short* img);
hipError_t launch_skip_rows_ln(const MlpFusedArgs& a, int D, hipStream_t s, bool with_ln = true);   // with_ln = false: x' only, column-split (D = 512)
size_t mlp_fused_partial_bytes(int max_batch, int extras, int D, int hidden);
void mlp_fused_plan(int B, int n_patches, int extras, int seq_len, int hidden, MlpFusedArgs& a);
void mlp_fused_pack(int D, int hidden, const float* w1, const float* b1, const float* w2, bool kperm,
                    unsigned short (*to_bf16)(float), unsigned short* img, float* b1p);
hipError_t launch_mlp_fused(const MlpFusedArgs& a, int D, hipStream_t s);
hipError_t launch_mlp_reduce(const MlpFusedArgs& a, int D, hipStream_t s);

// ---- row-resident Linear + bias + residual + LayerNorm for embed_dim 768 (rowlin.hip): x += A . W^T + b ; LayerNorm(x) g + beta as bf16
struct RowLinArgs {
    const bf16_t* A;       // [rows, lda] bf16 rows of the Linear's input (k contiguous)
    const bf16_t* A2;      // k_split > 0: the input is cat[A | A2] along k (skip_linear): k >= k_split comes from A2 [rows, lda]
    int k_split;           // a multiple of 64, or 0
    int set_x;             // != 0: x = A . W^T + b (no residual: skip_linear), else x += ...
    int lda, K;            // K % 64 == 0
    const char* wimg;      // rowlin_pack image of W [768, K]
    const float* bias;     // [768]
    float* xres;           // fp32 [rows, 768] residual stream, updated in place
    const float *ln_g, *ln_b;   // LayerNorm of the updated rows (h_out / h_frag)
    bf16_t* h_out;         // row-major [rows, 768] bf16, or null
    bf16_t* h_frag;        // or: the main (patch) rows in MFMA fragment order (MlpFusedArgs::ln_out_frag), or null
    bf16_t* x_copy;        // optional bf16 copy of the updated rows, row-major
    float* partial;        // slabs of the K-split extra-token tiles [tiles_extra * groups][128][768] fp32
    int M;                 // plain mode (tok_n == 0): rows [0, M) in tiles of 128
    // row plan (rowlin_plan; tok_n > 0): token row of image b, token l = b * tok_l + l; tokens [0, tok_e) are the extras, then tok_n patches
    int tok_n, tok_e, tok_l, n_main, n_extra, tiles_main, tiles_extra, groups, cpg;
};
bool rowlin_supported(int D, int K);
void rowlin_pack(int K, const float* w, unsigned short (*to_bf16)(float), unsigned short* img);
void rowlin_plan(int B, int n_patches, int extras, int seq_len, int K, RowLinArgs& a);
size_t rowlin_partial_bytes(int max_batch, int extras, int K);
hipError_t launch_rowlin(const RowLinArgs& a, hipStream_t s);

struct EmbedArgs {
    const float* x_img;      // [B,C,S,S]
    const float* wt;         // [pd, D]  patch-embed weight, transposed
    const float* bias;       // [D]
    const float* pos;        // [L, D]
    const float* label_emb;  // [num_classes, D] or null
    const long long* y;      // [B] or null
    const float* t_vec;      // [B] per-row timesteps or null (then st->t_model)
    StepState* st;           // t_model is read, t_final is written (block 0)
    float* x_tok;            // [Mp, D]
    int B, C, S, P, D, L, extras, num_classes, normalize, Mp;
    int generic;             // != 0: the generic VALU kernel even where the MFMA kernel fits (development A/B runs)
    const float* ln_g = nullptr;   // with ln_frag: the first block's norm1 of the patch rows is written too (embed_ln_supported)
    const float* ln_b = nullptr;
    bf16_t* ln_frag = nullptr;     // MFMA fragment order (launch_layernorm_frag's `frag`)
};
bool embed_mfma_ok(const EmbedArgs& a, size_t& lds);     // the MFMA kernel takes the shape; lds = the bytes its launch asks for
bool embed_ln_supported(const EmbedArgs& a);

// finishes a split-K Linear (launch_gemm_splitk) and runs the LayerNorm behind it: rowops.hip reduce_ln_kernel
struct ReduceLnArgs {
    float* x;               // fp32 [rows, D] residual stream (read when resid != 0, written always)
    const float* partial;   // fp32 slabs [splits][slab elements], row-major [rows, D] each
    long long slab;         // elements per slab (the GEMM's M * N)
    int splits, resid;
    const float* bias;      // [D]
    bf16_t* copy;           // optional bf16 copy of the updated rows, row stride ldo
    int ldo;
    const float *ln_g, *ln_b;   // optional LayerNorm of the updated rows ...
    bf16_t* h;              // ... row-major [rows, D] (with frag: only the extra-token rows go here)
    bf16_t* frag;           // ... or: the patch rows in MFMA fragment order (launch_layernorm_frag's `frag`)
    int tok_l, tok_e;
    int rows;
};
hipError_t launch_reduce_ln(const ReduceLnArgs& a, int D, hipStream_t s);
hipError_t launch_embed(const EmbedArgs& a, hipStream_t s);

// time_embed MLP (models/uvit.py:264-272): time token = W2 . SiLU(W1 . sinusoid(t) + b1) + b2 (+ pos_embed), fp32, one
// workgroup per image; overwrites the time-token row the embed kernel wrote.  w1t [D, 4D], w2t [4D, D]: transposed on the host.
struct TimeMlpArgs {
    const float *w1t, *b1, *w2t, *b2, *pos, *t_vec;
    const StepState* st;
    float* x_tok;
    int B, D, L, extras, normalize;
};
hipError_t launch_time_mlp(const TimeMlpArgs& a, hipStream_t s);

template <typename T>
hipError_t launch_layernorm(const float* x, const float* gamma, const float* beta, T* out,
                            int rows, int D, hipStream_t s);
hipError_t launch_layernorm_frag(const float* x, const float* gamma, const float* beta, bf16_t* out, bf16_t* frag, int rows, int D,
                                 int tok_l, int tok_e, hipStream_t s);   // patch rows in MFMA fragment order (MlpFusedArgs::ln_out_frag)

// qkv: head-major (HeadMajor, make_head_major(L, H)); out: [B * L, D] rows
template <typename T>
hipError_t launch_attention(const T* qkv, T* out, int B, int L, int H, int D, hipStream_t s);
// the same operands for 1 <= L <= kMaxLongL (4096 patches + 2 extra tokens): K / V stream through LDS in key blocks, online softmax
// (attention.hip attention_long_kernel).  The model takes it where L > 288 only; launch_attention and launch_v_copy keep their bound.
constexpr int kMaxLongL = 4098;
template <typename T>
hipError_t launch_attention_long(const T* qkv, T* out, int B, int L, int H, int D, hipStream_t s);
// attn.qkv + attention in one launch (attention.hip qkv_attention_kernel): h = norm1 of the patch rows in fragment order
// (MlpFusedArgs::ln_out_frag); the extra-token rows: hx = norm1 row-major [B L, D], or hx = nullptr and xres / ln_g / ln_b = the fp32
// residual stream and this block's norm1 parameters (the kernel normalises the rows itself); wimg from qkv_attention_pack;
// bf16, D = 512 / 768 / 1024 (heads of 64), L = 256 + extras, extras = 1 or 2 only (qkv_attention_supported); out_frag or null: the patch rows'
// output goes there in fragment order (MlpFusedArgs::ao_frag, B * 256 * D elements) instead of out, which then receives the extra-token rows only
bool qkv_attention_supported(int D, int H, int L, int extras);
void qkv_attention_pack(int D, int H, const float* w, unsigned short (*to_bf16)(float), unsigned short* img);
hipError_t launch_qkv_attention(const bf16_t* h, const bf16_t* wimg, const float* bias, const bf16_t* hx, const float* xres,
                                const float* ln_g, const float* ln_b, bf16_t* out, int B, int L, int H, int D, int extras, hipStream_t s,
                                bf16_t* out_frag = nullptr);

// Identity attention (perturbed-attention guidance): attention(q, k, v) = v for the B images given.  launch_v_identity is the companion of
// launch_qkv_attention (the same operands, xres / ln_g / ln_b mode only; qkv_attention_supported shapes): v is computed from norm1 and the
// v tiles of the weight image.  launch_v_copy is the companion of launch_attention: out [B L, D] rows = the v rows of the head-major qkv
// tensor, copied bit for bit (rows [L, Lp) of a unit are never read).
hipError_t launch_v_identity(const bf16_t* h, const bf16_t* wimg, const float* bias, const float* xres, const float* ln_g, const float* ln_b,
                             bf16_t* out, int B, int L, int H, int D, int extras, hipStream_t s);
template <typename T>
hipError_t launch_v_copy(const T* qkv, T* out, int B, int L, int H, int D, hipStream_t s);

struct FinalArgs {
    const float* dec;      // [B*L, pd] decoder_pred output for every token (extras included)
    const float* wconv;    // [C, C, 3, 3]
    const float* bconv;    // [C]
    const float* x_in;     // [B,C,S,S] or null (forward only)
    const float* z;        // [B,C,S,S] or null
    float* eps_out;        // or null
    float* x_out;          // or null (may alias x_in)
    StepState* st;         // reads t_final / seed; advance != 0: one thread sets t = t_final - 1 for the next step
    const StepCoef* coef;  // [1000]
    int B, C, S, P, L, extras, noise_mode, variance;
    int advance;
    const AffineRow* atab; // or null.  Set: st->t is a STEP INDEX k into this table; the update is a x + b eps + c z with row k,
                           // and advance hands row k + 1's timestep to the next step (the table holds one row more than steps)
    int b0 = 0;            // index of this launch's first image within the whole batch (a half-batch chain of dd_sample): only the
                           // Philox pixel ids depend on it, so that a chain draws the z the undivided batch would
    int layer_B = 0;       // > 0: the B "images" are layer_B images of B / layer_B early-exit layers, one after the other (dec, eps_out contiguous that way);
    long long w_stride = 0, b_stride = 0;   //   layer i convolves with wconv + i * w_stride / bconv + i * b_stride (floats): ONE launch for every layer's head
    // classifier-free guidance (pair_B > 0): dec holds 2 pair_B images, image b's conditional rows first and its unconditional rows at b + pair_B;
    // the grid covers the B = pair_B images, eps = eps_c + guide_scale * (eps_c - eps_u) goes through the update, x_in [b] is read and x_out [b]
    // AND x_out [b + pair_B] are written (the next step's unconditional rows then hold their input); z, eps_out: [B, C, S, S]; layer_B must be 0
    float guide_scale = 0.f;
    int pair_B = 0;
    // multistep loop (htab != null, atab set): row k of htab adds d h to the update when its hist flag is set, and h' = p x + q m is
    // written on every step; h [B, C, S, S] holds this launch's B images (guided: the conditional images only), x_out must be set
    const HistRow* htab = nullptr;
    float* h = nullptr;
    // the second halo's own source (guided launches).  Classifier-free guidance leaves these unset: launch_final derives them from dec,
    // pair_B and the one conv.  Autoguidance (pair_B == 0, dec2 set): dec2 [B * L2, pd] is the GUIDE model's decoder output for the same B
    // images (its own token count L2 / extras2, the same patch grid), convolved with the guide's wconv2 / bconv2;
    // eps = eps_main + guide_scale * (eps_main - eps_guide) goes through the update and x_out [b] alone is written; layer_B must be 0
    const float* dec2 = nullptr;
    const float* wconv2 = nullptr;
    const float* bconv2 = nullptr;
    int L2 = 0, extras2 = 0;
    // known region (kx0 != null; x_out set, layer_B == 0): x' is finished by step_update.h known() before it is stored, from the known image
    // kx0 [B, C, S, S], the mask kmask [B, 1, S, S] of this launch's B images and row t of ktab (the DDPM loop: 1000 rows by timestep; a
    // table-driven loop: beside atab); z2 is a Philox draw of its own (noise_mode 2), no other noise mode adds one.  Guided, the twin gets x'' too.
    const float* kx0 = nullptr;
    const float* kmask = nullptr;
    const KnownRow* ktab = nullptr;
    // per-image seeds (dd_set_image_seeds) of the WHOLE batch, or null: image b of this launch draws z / z2 under seeds[b0 + b] with
    // image-local pixel ids (step_update.h draw_site); null: st->seed and the batch-wide pixel ids
    const unsigned long long* seeds = nullptr;
};
hipError_t launch_final(const FinalArgs& a, hipStream_t s);

// final LayerNorm + decoder_pred in one launch (rowops.hip); wg = decoder weight * norm gamma [pd, D], c = decoder bias + W . norm beta
struct HeadDecArgs {
    const float* x;    // [Mp, D] fp32 residual stream
    const float* wg;   // [pd, D]
    const float* c;    // [2 pd]: c, then the row sums of wg (the kernel multiplies the un-normalised rows: rowops.hip)
    float* dec;        // [Mp, pd]
    int M, pd;
    int tok_l, tok_e;  // > 0: rows are images of tok_l tokens whose first tok_e (the extra tokens) are NOT decoded; 0: every row
    // early-exit MLP probe folded into the launch (srow != null; D = 256 / 512): srow[row] = sigmoid(x[row,:] . w + b) for EVERY row (the extra
    // tokens' too), w = pw_base + pi D, b = pb_base[pi], pi = st->t_final * t_mul + add (launch_ee_probe's row selection)
    float* srow = nullptr;
    const float* pw_base = nullptr;
    const float* pb_base = nullptr;
    const StepState* st = nullptr;
    int t_mul = 0, add = 0;
    int split = 0;     // 1: wg is the packed split-bf16 image (pack_head_split) and c's row sums are of hi + lo; D = 256 / 512 (rowops.hip: SPLIT)
};
bool head_dec_probe_supported(int D);
// Wg [pd, D] -> the SPLIT kernel's image: [jj < D / 32][ct < nt][hi, lo][64 lanes] x 8 bf16 (2 D nt 16 bf16 = the fp32 matrix's bytes at pd = 16 nt);
// wsum [pd]: the row sums of hi + lo (what the kernel multiplies)
void pack_head_split(int D, int pd, const float* wg, unsigned short (*f2bf)(float), unsigned short* img, float* wsum);
bool head_dec_supported(int D, int pd);
hipError_t launch_head_dec(const HeadDecArgs& a, int D, int num_cus, hipStream_t s);

hipError_t launch_ddpm_step(const float* x, const float* eps, const float* z, float* out,
                            StepCoef c, int use_noise, long long n, hipStream_t s);
template <typename T> hipError_t launch_fill_random(T* p, long long n, unsigned seed, float scale, hipStream_t s);
// ---- KL-VAE decoder / encoder bandwidth kernels (vae_kernels.hip)
hipError_t launch_vae_input(const float* z, const float* w, const float* b, float inv_scale, float* out, int B, int HW, hipStream_t s);
hipError_t launch_vae_output(const float* in, float* out, int B, int C, int HW, int ldc, hipStream_t s);
template <typename T> hipError_t launch_im2col3x3(const T* src, T* dst, int B, int H, int W, int C, int up, int Kpad, hipStream_t s);
// Downsample's gather: src [B, 2H, 2W, C] -> rows of the H x W output, pad on the bottom / right only
template <typename T> hipError_t launch_im2col3x3_s2(const T* src, T* dst, int B, int H, int W, int C, int Kpad, hipStream_t s);
hipError_t launch_vae_image(const float* x, float* out, int B, int HW, hipStream_t s);      // [B,3,HW] NCHW -> [B*HW, 4], channel 3 zero
// h [B*HW, 8] -> quant_conv (w [8, 8], b [8]) -> moments [B,8,HW] and / or z [B,4,HW] (either may be null; eps null: z = scale * mean)
hipError_t launch_vae_moments(const float* h, const float* w, const float* b, const float* eps, float* moments, float* z, int B, int HW,
                              hipStream_t s);
hipError_t launch_vae_sample(const float* moments, const float* eps, float* z, int B, int HW, hipStream_t s);
template <typename T> hipError_t launch_im2col3x3_c4(const float* src, T* dst, int B, int H, int W, int Kpad, hipStream_t s);
template <typename T> hipError_t launch_groupnorm(const float* x, float* part, const float* gamma, const float* beta, T* out, int B, int HW, int C, int swish, hipStream_t s);
int groupnorm_partials(int B, int HW);
template <typename T> hipError_t launch_softmax_rows(const float* sc, T* p, long long rows, int n, float scale, hipStream_t s);
template <typename T> hipError_t launch_cast(const float* x, T* out, long long n, hipStream_t s);

hipError_t launch_affine_step(const float* x, const float* m, const float* z, float* out, float a, float b, float c,
                              long long n, hipStream_t s);
// out = a x + b m [+ d h if use_hist] [+ c z if z], h = p x + q m (read before it is written): the multistep row, elementwise
hipError_t launch_multistep_step(const float* x, const float* m, const float* z, float* h, float* out, float a, float b, float c, float d,
                                 float p, float q, int use_hist, long long n, hipStream_t s);
// out = known(x, x0, mask, ka, kb, z2) elementwise on [B, C, S, S] (mask [B, 1, S, S]; z2 null: none): the unfused known-region rule
hipError_t launch_known_blend(const float* x, const float* x0, const float* mask, const float* z2, float ka, float kb, float* out, int B, int C,
                              int S, hipStream_t s);
// x0 thresholding of a multistep step (step_update.h; include/duodiff.h dd_x0_threshold) as the kernel takes it
struct X0Threshold {
    int dynamic;            // 0: static, xh = clamp(x0, +-range); 1: dynamic, the image's own scale s
    int i;                  // dynamic: floor(quantile (n - 1)) in double on the host, n = C S S
    float f;                //          and (float)(quantile (n - 1) - i)
    float range, s_max;
};
constexpr int THRESHOLD_MAX_ELEMS = 16384;    // one image's x0 lives in LDS (64 KB)
// The thresholded multistep step on B images [B, C, S, S], one workgroup per image: x0 = p x + q m, the image's scale, xh, then
// x' = a x + b xh [+ d h] [+ c z], h' = xh, x' finished by the known region where one is given.  Two ways to name the row:
//   st set:  the loop -- row st->t_final of atab / htab (/ ktab), noise_mode 0 / 2 (Philox: batch-wide pixel ids from b0), advance as
//            FinalArgs::advance; pair_B > 0 stores x' to image b + pair_B too (classifier-free guidance)
//   st null: dd_threshold_step -- the row by value (row, hr), z a buffer or null
struct ThresholdArgs {
    const float* x; const float* m; const float* z; float* h; float* out;
    StepState* st = nullptr;
    const StepCoef* coef = nullptr;
    const AffineRow* atab = nullptr;
    const HistRow* htab = nullptr;
    AffineRow row{};
    HistRow hr{};
    int noise_mode = 0, advance = 0, b0 = 0, pair_B = 0;
    const float* kx0 = nullptr;
    const float* kmask = nullptr;
    const KnownRow* ktab = nullptr;
    X0Threshold thr{};
    int B = 0, C = 0, S = 0;
    const unsigned long long* seeds = nullptr;     // as FinalArgs::seeds (the loop only)
};
hipError_t launch_threshold_step(const ThresholdArgs& a, hipStream_t s);

// AttentionProbe operands of one layer (model.hip finalize folds them): u [D], Wv^T [D, D], bv [D], W0^T [D, D], b0 [D], w2 [D], b2 [1]
struct AttnProbeW { const float *u, *wvt, *bv, *w0t, *b0, *w2, *b2; };
hipError_t launch_ee_attn_probe(const float* x, const AttnProbeW& w, float* out, int B, int L, int D, hipStream_t s);
// probe row = (t_mul ? st->t_final * t_mul : 0) + add of the [n_probe, D] / [n_probe] tables; srow: [B, L] fp32 scratch (the rows' sigmoids)
hipError_t launch_ee_probe(const float* x, const float* w_base, const float* bias_base, float* out, float* srow, int B, int L, int D,
                           const StepState* st, int t_mul, int add, hipStream_t s);
hipError_t launch_ee_probe_reduce(const float* srow, float* out, int rows, int L, hipStream_t s);   // out == nullptr above: the rows only; this finishes any number of (layer, image) rows
// dd_early_exit_select: mo [B, chw] = the selected output, idx [B] (or null), err_mean [depth] = the per-layer mean of cls over the batch (or null)
hipError_t launch_ee_select(const float* outs, const float* eps, const float* cls, float thr, int depth, int B, long long chw,
                            float* mo, int* idx, float* err_mean, hipStream_t s);
// the selection and the DDPM update in one launch (the device-resident loop): idx / err_mean are [1000, idx_stride] / [1000, depth] tables and row
// st->t_final is written.  A half-batch chain: B = the chain's images, idx_col0 = its first image within the whole batch (its idx columns,
// its Philox pixel ids); sums: err_mean receives the plain per-layer SUM over the chain's images (launch_ee_mean_combine joins the chains);
// seeds: the whole batch's per-image seeds (FinalArgs::seeds) or null
hipError_t launch_ee_select_step(float* x, const float* outs, const float* eps, const float* cls, float thr, int depth, int* idx, float* err_mean,
                                 int idx_stride, int idx_col0, bool sums, StepState* st, const StepCoef* coef, int B, int C, int S,
                                 int noise_mode, int advance, hipStream_t s, const unsigned long long* seeds = nullptr);
// out [B, C, S, S] = the x_T draw of step_update.h (PHILOX_START) under `seed` (seeds null) or the per-image seeds [B]; C in 1..4; a bad
// argument is hipErrorInvalidValue with nothing launched
hipError_t launch_noise_images(float* out, const unsigned long long* seeds, unsigned long long seed, int ctr, int B, int C, int S, hipStream_t s);
// A resampling jump of a table-driven loop, in place on B images x [B, C, S, S] whose first is image b0 of the whole batch (seeds as
// FinalArgs::seeds): x' = a x [+ c z3] from row st->t of atab (step_update.h jump), written to the twin image pair_B images on as well
// (pair_B > 0: classifier-free guidance); a second, one-thread launch then hands row st->t + 1 its index and t_model.  C outside 1..4 or a
// null pointer: hipErrorInvalidValue, nothing launched.
hipError_t launch_jump(float* x, StepState* st, const AffineRow* atab, const unsigned long long* seeds, int B, int C, int S, int b0, int pair_B,
                       int noise_mode, hipStream_t s);
// out = ja x [+ jc z if z] on n elements: the unfused jump (x and out may alias)
hipError_t launch_jump_step(const float* x, const float* z, float* out, float ja, float jc, long long n, hipStream_t s);
// Block caching (cache.hip): out = last + w (last - prev) on n elements of the activation type (n % 64 == 0, 16-byte aligned, out aliasing
// neither input).  atab set: the op and w of row st->t (AffineRow::pad1 = the op, pad2 = the bits of w); else the arguments.  op 2
// extrapolates, any other op copies last and does not read prev.  The grid holds at most CACHE_MAX_BLOCKS workgroups of 256 and strides.
enum { CACHE_REFRESH = 0, CACHE_REUSE = 1, CACHE_EXTRAPOLATE = 2 };
constexpr int CACHE_MAX_BLOCKS = 2048;
hipError_t launch_cache_extrapolate(const void* last, const void* prev, void* out, long long n, bool bf16, const StepState* st,
                                    const AffineRow* atab, int op, float w, hipStream_t s);
hipError_t launch_ee_mean_combine(const float* s0, const float* s1, float* err, int depth, int t_lo, int t_hi, int B, hipStream_t s);
hipError_t launch_set_state(StepState* st, int t, unsigned long long seed, hipStream_t s);
hipError_t launch_set_state_table(StepState* st, const AffineRow* atab, unsigned long long seed, hipStream_t s);   // step index 0
hipError_t launch_set_state_float(StepState* st, float t, hipStream_t s);
// ---- the denoising-error scan (scan.hip), B images [B, C, S, S] of a whole batch of B_all whose first is image b0; seeds as FinalArgs::seeds.
// Both follow the step-state contract: diffuse is the step's FIRST kernel (row st->t), error its LAST (row st->t_final; advance != 0: one
// thread hands on t + 1 and row t + 1's t_model).  C outside 1..4, C S S > 2^24 or a null pointer: hipErrorInvalidValue, nothing launched.
hipError_t launch_scan_diffuse(const float* x0, float* xt, const StepState* st, const ScanRow* tab, const unsigned long long* seeds, int B, int C,
                               int S, int b0, hipStream_t s);                       // xt = ka x0 + kb z
hipError_t launch_scan_error(const float* x0, const float* m, float* err, StepState* st, const ScanRow* tab, const unsigned long long* seeds,
                             int B, int C, int S, int b0, int B_all, int advance, hipStream_t s);   // err[t_final B_all + b0 + b]
hipError_t launch_set_state_scan(StepState* st, const ScanRow* tab, unsigned long long seed, hipStream_t s, int row = 0);   // t = t_final = row
// The early-exit scan's last kernel: `exits` = depth + 1 outputs of one forward (outs [exits - 1, B, C, S, S], eps [B, C, S, S], cls [exits - 1, B];
// exits == 1: eps alone, outs / cls / pred may be null) against the one target; the row is tab[st->t_final], a table indexed by TIMESTEP, the
// output row is row.ctr - tab[SCAN_EXITS_ROWS].ctr (that row's ctr: the call's counter_base): mse, tgtu [.., exits, B_all], pred [.., exits - 1, B_all] at column b0 + b.  advance != 0: one thread hands on
// t = row.next and that row's t_model.  C outside 1..4, C S S > 2^24, exits outside 1..32, a null pointer: hipErrorInvalidValue, nothing launched.
hipError_t launch_scan_exits_error(const float* x0, const float* outs, const float* eps, const float* cls, float* mse, float* tgtu, float* pred,
                                   StepState* st, const ScanRow* tab, const unsigned long long* seeds, int B, int C, int S, int exits, int b0,
                                   int B_all, int advance, hipStream_t s);
constexpr int SCAN_EXITS_ROWS = 1000;      // the early-exit scan's table: rows 0 .. 999 by timestep, row 1000 the base row
hipError_t launch_guided_labels(const long long* y, long long* out, int B, long long null_label, hipStream_t s);   // out [2 B] = [y [0, B) | null_label x B]
// (x + 1) / 2, NCHW -> NHWC: the output convention of reference sampler.py:145-146
hipError_t launch_to_images(const float* x, float* out, int B, int C, int S, hipStream_t s);

}  // namespace dd
