// What the projection GEMM family shares (gemm_bf16.hip: 64 / 96 / 128-row tiles on 16x16x32 MFMAs; gemm_big.hip: 256 x 256
// tiles on 32x32x16 MFMAs; gemm_bnsilu.hip: BatchNorm + SiLU on the A operand; gemm_fp8.hip / gemm_mxfp8.hip: row-scaled and
// block-scaled e4m3 operands): the epilogue arguments and the per-vector epilogue, the two tile epilogues through LDS, the
// XCD-aware tile order with its grid size, the operand checks of the extern "C" entries, and the main loop of the
// register-staged kernels (clamped 16-byte loads, the per-thread register tile, the load / MFMA / store skeleton, the 16x16x32
// bf16 MFMA step) with the two LDS-DMA helpers of the others.  A kernel's own: what it stages that is not a plain K-contiguous
// tile (the implicit-GEMM gather, the BatchNorm + SiLU on the way into LDS, the MX scale words), the fp8 MFMAs, and the stage
// rings of the LDS-DMA kernels.
#pragma once
#include <hip/hip_bf16.h>

#include <type_traits>

#include "dropout_mask.h"
#include "ia_common.h"

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int GEMM_THREADS = 256;   // 4 waves, 2 x 2 over the tile

// out = alpha * dropout(act(acc + bias)) + R: the epilogue every kernel of the family has
struct GemmEpi {
    const float* bias; const float* R;
    float* outF; __bf16* outH;
    int M, N, ldr, ldof, ldoh;
    int act;            // 0 none, 1 SiLU, 2 ReLU; GemmArgs only: 3 SiLU backward against aux, 4 GLU
    float alpha;
    unsigned seed, thr; // dropout keep if byte >= thr, survivors scaled by keep_scale (ia_dropout_rule)
    float keep_scale;
};

// The bf16 kernels' operands and what only their entries offer
struct GemmArgs : GemmEpi {
    const __bf16* A; const __bf16* W;
    int K, lda, ldw;
    __bf16* outPre;     // optional: the bias-added value BEFORE act / dropout, rounded to bf16 (the activation is then applied
                        // to the rounded value: what a separate elementwise pass over outPre would compute)
    const __bf16* aux;  // act == 3: out = bf16(acc) * SiLU'(aux) -- the data gradient through dropout(SiLU(.)) in one pass
    int ldpre, ldaux;
    int out_f16;        // outH holds IEEE half instead of bf16 (the joint's f16 operands come straight out of its projections)
    // implicit-GEMM mode (CONV): A is a channels-last image [cB, cT1, cF1, cC]; row m = (b, t2, f2) of the 3x3 / stride-2 /
    // pad-1 convolution output [cB, cT2, cF2, N]; k = tap*cC + ci.
    int cT1, cF1, cC, cT2, cF2;
    // LayerNorm of the finished row (64 x 256 tiles, N == 256 only: a workgroup owns whole rows): outF keeps the updated
    // residual, outH receives LN(row) * ln_g + ln_b as bf16 -- the next projection's operand
    const float* ln_g; const float* ln_b; float ln_eps;
};

// 8 consecutive output columns gn .. gn+7 of row gm: v = the accumulated products.  bias -> (outPre) -> activation ->
// dropout -> alpha -> residual -> fp32 and / or bf16 / f16 stores, all 16-byte accesses.  Args = GemmArgs or any other
// extension of GemmEpi; what only GemmArgs carries is compiled for GemmArgs alone.
template <class Args>
__device__ __forceinline__ void gemm_epilogue8(const Args& a, int gm, int gn, float (&v)[8]) {
    constexpr bool FULL = std::is_same<Args, GemmArgs>::value;
    if (a.bias) {
        const float4 b0 = *reinterpret_cast<const float4*>(a.bias + gn), b1 = *reinterpret_cast<const float4*>(a.bias + gn + 4);
        v[0] += b0.x; v[1] += b0.y; v[2] += b0.z; v[3] += b0.w; v[4] += b1.x; v[5] += b1.y; v[6] += b1.z; v[7] += b1.w;
    }
    if constexpr (FULL) {
        if (a.outPre) {
            union { uint4 u; __bf16 h[8]; } o;
#pragma unroll
            for (int j = 0; j < 8; ++j) { o.h[j] = (__bf16)v[j]; v[j] = (float)o.h[j]; }
            *reinterpret_cast<uint4*>(a.outPre + (size_t)gm * a.ldpre + gn) = o.u;
        }
    }
    if (a.act == 1) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = ia_silu_fast(v[j]);
    } else if (a.act == 2) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = fmaxf(v[j], 0.f);
    } else if constexpr (FULL) {
        if (a.act == 3) {
            union { uint4 u; __bf16 h[8]; } x;
            x.u = *reinterpret_cast<const uint4*>(a.aux + (size_t)gm * a.ldaux + gn);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float t = (float)x.h[j], sg = ia_sigmoid_fast(t);
                v[j] = (float)(__bf16)v[j] * (sg * (1.f + t * (1.f - sg)));
            }
        }
    }
    float sc_all = a.alpha;
    if (a.thr > 0) {
        const unsigned m = ia_keep8(a.seed, (unsigned)gm, (unsigned)a.N, (unsigned)gn, a.thr);
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (!((m >> j) & 1u)) v[j] = 0.f;
        sc_all *= a.keep_scale;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] *= sc_all;
    if (a.R) {
        const float4 r0 = *reinterpret_cast<const float4*>(a.R + (size_t)gm * a.ldr + gn);
        const float4 r1 = *reinterpret_cast<const float4*>(a.R + (size_t)gm * a.ldr + gn + 4);
        v[0] += r0.x; v[1] += r0.y; v[2] += r0.z; v[3] += r0.w; v[4] += r1.x; v[5] += r1.y; v[6] += r1.z; v[7] += r1.w;
    }
    if (a.outF) {
        *reinterpret_cast<float4*>(a.outF + (size_t)gm * a.ldof + gn) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4*>(a.outF + (size_t)gm * a.ldof + gn + 4) = make_float4(v[4], v[5], v[6], v[7]);
    }
    bool f16 = false, store_h = a.outH != nullptr;
    if constexpr (FULL) { f16 = a.out_f16; store_h = a.outH && !a.ln_g; }
    if (store_h) {
        if (f16) {
            union { uint4 u; _Float16 h[8]; } o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o.h[j] = (_Float16)v[j];
            *reinterpret_cast<uint4*>(a.outH + (size_t)gm * a.ldoh + gn) = o.u;
        } else {
            union { uint4 u; __bf16 h[8]; } o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o.h[j] = (__bf16)v[j];
            *reinterpret_cast<uint4*>(a.outH + (size_t)gm * a.ldoh + gn) = o.u;
        }
    }
}

// XCD-aware tile order: workgroup ids go round-robin over the 8 XCDs, so the column tiles that share one row tile of A are
// given ids congruent mod 8 and consecutive in that XCD's dispatch order -- the A tile is then fetched into ONE XCD's L2 once
// instead of into all eight (W is small and lives in every L2).  Row tiles are padded to a multiple of 8: false for the
// padding workgroups of the last group (uniform).
template <int BM, int BN>
__device__ __forceinline__ bool gemm_xcd_tile(int M, int N, int& m0, int& n0) {
    const int ntn = (N + BN - 1) / BN;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int mt = xcd + 8 * (slot / ntn);
    m0 = mt * BM; n0 = (slot % ntn) * BN;
    return m0 < M;
}
inline int gemm_xcd_grid(int M, int N, int BM, int BN) {
    const int ntm = (M + BM - 1) / BM, ntn = (N + BN - 1) / BN;
    return 8 * ((ntm + 7) / 8) * ntn;
}

// ---- Register-staged operand tiles: ONE LDS stage of 144-byte rows (a 128-byte k-tile = 64 bf16 or 128 e4m3, + 16 bytes of
// padding: conflict-free 16-byte fragment reads), the next k-tile prefetched in registers while the MFMAs run on the current one.
// The staging registers are plain arrays indexed by fully unrolled loops and captured by the kernels' lambdas: they stay in
// VGPRs (0 bytes of scratch in every kernel that uses them, profiles/gemm_staging_refactor.md).
constexpr int GEMM_ROWB = 128 + 16;

// 16 bytes at element k of a K-contiguous row; elements at and past K read as zero (K % 8 == 0 for bf16, % 16 for e4m3: d_model =
// 144 is two 64-wide k-tiles and a 16-wide tail).  The address is clamped, the select applied to the value: no branch around the load.
template <class T>
__device__ __forceinline__ uint4 gemm_load16_k(const T* row, int k, int K) {
    const uint4 v = *reinterpret_cast<const uint4*>(row + (k < K ? k : 0));
    return k < K ? v : make_uint4(0, 0, 0, 0);
}

// A thread's share of a ROWS-row operand tile: vector i = tile row (tid + i * GEMM_THREADS) >> 3, 16-byte column (tid & 7).  Rows
// past the limit are clamped to the last valid one (their products land in output rows / columns that the epilogue never stores).
// K_TAIL = false: the caller guarantees whole k-tiles; the loads are then unconditional (the compiler turns the k-tail select into
// a branch around each load, which the kernel of the double-rate MFMA cannot hide).  Every vector is assigned from a by-value
// temporary: a whole-struct copy `v[i] = *ptr` straight from memory is what leaves the array in scratch.
template <int ROWS, bool K_TAIL = true>
struct GemmRegTile {
    static constexpr int NV = ROWS * 8 / GEMM_THREADS;
    static_assert(NV * GEMM_THREADS == ROWS * 8, "whole vectors per thread");
    uint4 v[NV];
    template <class T>
    __device__ __forceinline__ void load(const T* base, int ld, int row0, int row_limit, int k0, int K) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = threadIdx.x + i * GEMM_THREADS, row = idx >> 3, k = k0 + (idx & 7) * (16 / (int)sizeof(T));
            const T* rowp = base + (size_t)((row0 + row < row_limit) ? (row0 + row) : (row_limit - 1)) * ld;
            if constexpr (K_TAIL) {
                v[i] = gemm_load16_k(rowp, k, K);
            } else {
                const uint4 t = *reinterpret_cast<const uint4*>(rowp + k);
                v[i] = make_uint4(t.x, t.y, t.z, t.w);
            }
        }
    }
    __device__ __forceinline__ void store(unsigned char* tile) const {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = threadIdx.x + i * GEMM_THREADS;
            *reinterpret_cast<uint4*>(tile + (idx >> 3) * GEMM_ROWB + (idx & 7) * 16) = v[i];
        }
    }
};

// The main loop of the register-staged kernels.  load(kt): k-tile kt global -> registers; store(kt): those registers -> the LDS
// stage; compute(kt): the MFMAs on the stage.  Called by all threads of the workgroup.
template <class Load, class Store, class Compute>
__device__ __forceinline__ void gemm_staged_loop(int nk, Load load, Store store, Compute compute) {
    load(0);
    store(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        if (kt + 1 < nk) load(kt + 1);
        compute(kt);
        __syncthreads();
        if (kt + 1 < nk) {
            store(kt + 1);
            __syncthreads();
        }
    }
}

// 16x16x32 bf16 MFMAs over one 64-deep k-tile of the stage: TI x TJ accumulator tiles of a wave.  sa / sb = the lane's fragment
// address in the first of its TI / TJ 16-row groups: tile + (first row + (lane & 15)) * GEMM_ROWB + (lane >> 4) * 16.
typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
template <int TI, int TJ>
__device__ __forceinline__ void gemm_mfma_bf16_ktile(const unsigned char* sa, const unsigned char* sb, f4 (&acc)[TI][TJ]) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        bf8 af[TI], bfr[TJ];
#pragma unroll
        for (int i = 0; i < TI; ++i) af[i] = *reinterpret_cast<const bf8*>(sa + i * 16 * GEMM_ROWB + ks * 64);
#pragma unroll
        for (int j = 0; j < TJ; ++j) bfr[j] = *reinterpret_cast<const bf8*>(sb + j * 16 * GEMM_ROWB + ks * 64);
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < TJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
}

// (LDS-DMA staging of gemm_bf16_nt_dma_kernel and gemm_big_kernel: ia_lds_dma_lane / ia_lds_dma16 in ia_common.h)

// sum over the 32 lanes of a half wave (as csrc/ffn_fused.hip): every lane of the half wave gets the total
__device__ __forceinline__ float gemm_half_wave_sum(float v) {
    v += IA_DPP_F(0.f, v, 0xB1, 0xF);    // quad_perm xor 1
    v += IA_DPP_F(0.f, v, 0x4E, 0xF);    // quad_perm xor 2
    v += IA_DPP_F(0.f, v, 0x141, 0xF);   // row_half_mirror
    v += IA_DPP_F(0.f, v, 0x140, 0xF);   // row_mirror
    v += __shfl_xor(v, 16, 64);
    return v;
}

// Tile rows per pass of the row-major tile epilogue: one LDS stage + a 64-row epilogue tile keep a 128-column workgroup at
// 37 KB (four workgroups per CU)
constexpr int gemm_epi_rows(int BM, int BN) { return (BN == 256) ? 32 : ((BM == 96) ? 48 : 64); }
constexpr int gemm_epi_bytes(int BM, int BN) { return gemm_epi_rows(BM, BN) * (BN + 4) * 4; }

// The tile epilogue of the kernels whose 2 x 2 waves hold [TI][TJ] row-major 16x16 accumulator tiles (lane (c, q) = column c,
// rows 4 q .. 4 q + 3): accumulators -> LDS (fp32, row-major, gemm_epi_rows tile rows per pass) -> row-major elementwise pass
// with 16-byte accesses (GemmArgs: GLU / LayerNorm variants included).  Called by ALL threads of the workgroup once the stages
// in `smem` are free.
template <int BM, int BN, class Args>
__device__ __forceinline__ void gemm_tile_epilogue(const Args& a, f4 (&acc)[BM / 32][BN / 32], unsigned char* smem, int m0, int n0) {
    constexpr bool FULL = std::is_same<Args, GemmArgs>::value;
    constexpr int WM = BM / 2, WN = BN / 2, TI = WM / 16, TJ = WN / 16;
    constexpr int LDC = BN + 4;
    constexpr int EP_ROWS = gemm_epi_rows(BM, BN);
    static_assert(BM % EP_ROWS == 0 && (EP_ROWS % WM == 0 || WM % EP_ROWS == 0), "epilogue passes cover whole wave rows");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, q = lane >> 4;
    const int wm = wave >> 1, wn = wave & 1;
    float* sc = reinterpret_cast<float*>(smem);
    constexpr int VEC_PER_ROW = BN / 8;
    for (int pass = 0; pass < BM / EP_ROWS; ++pass) {
    if (pass > 0) __syncthreads();
    if ((wm * WM) / EP_ROWS == pass) {
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < TJ; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    sc[(wm * WM - pass * EP_ROWS + i * 16 + q * 4 + r) * LDC + wn * WN + j * 16 + c] = acc[i][j][r];
    }
    __syncthreads();
    if constexpr (FULL) {
    if (a.act == 4) {
        // GLU over the tile's column halves (weight rows regrouped by the caller: columns [0,64) of a 128-column tile are value
        // channels, [64,128) their gates): out[gm][n0/2 + c] = (v + b) * sigmoid(g + b'), bf16, N/2 columns wide.  Thread = 4
        // channels of one row: float4 reads of both halves, one 8-byte store, every thread busy.
        if constexpr (BN == 128) {
            for (int it = tid; it < EP_ROWS * 16; it += GEMM_THREADS) {
                const int row = it >> 4, cg = it & 15;
                const int gm = m0 + pass * EP_ROWS + row, gc = n0 + cg * 4;
                if (gm >= a.M) continue;
                float4 vv = *reinterpret_cast<const float4*>(sc + row * LDC + cg * 4);
                float4 gg = *reinterpret_cast<const float4*>(sc + row * LDC + 64 + cg * 4);
                if (a.bias) {
                    const float4 bv = *reinterpret_cast<const float4*>(a.bias + gc), bg = *reinterpret_cast<const float4*>(a.bias + gc + 64);
                    vv.x += bv.x; vv.y += bv.y; vv.z += bv.z; vv.w += bv.w;
                    gg.x += bg.x; gg.y += bg.y; gg.z += bg.z; gg.w += bg.w;
                }
                union { uint2 u; __bf16 h[4]; } o;
                o.h[0] = (__bf16)(vv.x * ia_sigmoid_fast(gg.x)); o.h[1] = (__bf16)(vv.y * ia_sigmoid_fast(gg.y));
                o.h[2] = (__bf16)(vv.z * ia_sigmoid_fast(gg.z)); o.h[3] = (__bf16)(vv.w * ia_sigmoid_fast(gg.w));
                *reinterpret_cast<uint2*>(a.outH + (size_t)gm * a.ldoh + (n0 >> 1) + cg * 4) = o.u;
            }
        }
        continue;   // next epilogue pass
    }
    }
    for (int it = tid; it < EP_ROWS * VEC_PER_ROW; it += GEMM_THREADS) {
        const int row = it / VEC_PER_ROW, cv = it - row * VEC_PER_ROW;
        const int gm = m0 + pass * EP_ROWS + row, gn = n0 + cv * 8;
        if (gm >= a.M || gn >= a.N) continue;
        float v[8];
        const float4 x0 = *reinterpret_cast<const float4*>(sc + row * LDC + cv * 8);
        const float4 x1 = *reinterpret_cast<const float4*>(sc + row * LDC + cv * 8 + 4);
        v[0] = x0.x; v[1] = x0.y; v[2] = x0.z; v[3] = x0.w; v[4] = x1.x; v[5] = x1.y; v[6] = x1.z; v[7] = x1.w;
        gemm_epilogue8(a, gm, gn, v);
        if constexpr (FULL && BN == 256) {
            // LayerNorm of the finished row: its 256 columns are the 32 lanes of this half wave (8 columns each; rows beyond M
            // skip the whole half wave above), two DPP / shuffle reductions, bf16 store of the normalised row
            if (a.ln_g) {
                float s1 = 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) s1 += v[j];
                const float mean = gemm_half_wave_sum(s1) * (1.f / 256.f);
                float s2 = 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) { v[j] -= mean; s2 += v[j] * v[j]; }
                const float rstd = rsqrtf(gemm_half_wave_sum(s2) * (1.f / 256.f) + a.ln_eps);
                const float4 g0 = *reinterpret_cast<const float4*>(a.ln_g + gn), g1 = *reinterpret_cast<const float4*>(a.ln_g + gn + 4);
                const float4 c0 = *reinterpret_cast<const float4*>(a.ln_b + gn), c1 = *reinterpret_cast<const float4*>(a.ln_b + gn + 4);
                const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
                const float bb[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
                union { uint4 u; __bf16 h[8]; } o;
#pragma unroll
                for (int j = 0; j < 8; ++j) o.h[j] = (__bf16)(v[j] * rstd * gg[j] + bb[j]);
                *reinterpret_cast<uint4*>(a.outH + (size_t)gm * a.ldoh + gn) = o.u;
            }
        }
    }
    }
}

// The tile epilogue of the fp8 kernels (128 x 128 tiles, 2 x 2 waves, product computed TRANSPOSED: lane (c, q) of accumulator
// tile [i][j] holds columns 16 j + 4 q .. + 3 of row 16 i + c): 16-byte writes into the fp32 LDS tile, 64 tile rows per pass,
// then the same row-major pass.  ROW_SCALED: per-row / per-column operand scales sa[M] / sw[N] are applied before the bias
// (x * sa[m] * sw[n], in this order); otherwise the operands carried their scales into the MFMA and sa / sw are not read.
constexpr int GEMM_T_BM = 128, GEMM_T_BN = 128;
constexpr int GEMM_T_EPI = 64 * (GEMM_T_BN + 4) * 4;   // bytes of the fp32 LDS tile: 33 792
template <bool ROW_SCALED, class Args>
__device__ __forceinline__ void gemm_tile_epilogue_t(const Args& a, f4 (&acc)[4][4], unsigned char* smem, int m0, int n0,
                                                     const float* sa = nullptr, const float* sw = nullptr) {
    constexpr int LDC = GEMM_T_BN + 4, VEC_PER_ROW = GEMM_T_BN / 8;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, q = lane >> 4;
    const int wm = wave >> 1, wn = wave & 1;
    float* sc = reinterpret_cast<float*>(smem);
    for (int pass = 0; pass < 2; ++pass) {
        if (pass) __syncthreads();
        if (wm == pass) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    *reinterpret_cast<float4*>(sc + (i * 16 + c) * LDC + wn * 64 + j * 16 + q * 4) =
                        make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
        }
        __syncthreads();
        for (int it = tid; it < 64 * VEC_PER_ROW; it += GEMM_THREADS) {
            const int row = it / VEC_PER_ROW, cv = it - row * VEC_PER_ROW;
            const int gm = m0 + pass * 64 + row, gn = n0 + cv * 8;
            if (gm >= a.M || gn >= a.N) continue;
            const float4 x0 = *reinterpret_cast<const float4*>(sc + row * LDC + cv * 8);
            const float4 x1 = *reinterpret_cast<const float4*>(sc + row * LDC + cv * 8 + 4);
            float v[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
            if constexpr (ROW_SCALED) {
                const float s_m = sa[gm];
                const float4 w0 = *reinterpret_cast<const float4*>(sw + gn), w1 = *reinterpret_cast<const float4*>(sw + gn + 4);
                v[0] = v[0] * s_m * w0.x; v[1] = v[1] * s_m * w0.y; v[2] = v[2] * s_m * w0.z; v[3] = v[3] * s_m * w0.w;
                v[4] = v[4] * s_m * w1.x; v[5] = v[5] * s_m * w1.y; v[6] = v[6] * s_m * w1.z; v[7] = v[7] * s_m * w1.w;
            }
            gemm_epilogue8(a, gm, gn, v);
        }
    }
}

// The operand checks the extern "C" entries have in common, then the epilogue arguments.  The order is part of the C ABI
// (callers tell IA_INVALID_VALUE from IA_UNSUPPORTED): presence, then what the kernels were not built for (`own_unsupported` =
// the entry's own conditions of that kind, leading dimensions), then alignment and the dropout probability.  An entry's own
// IA_INVALID_VALUE checks go in front of or behind the call.
inline int gemm_check_and_fill(GemmEpi& e, const void* A, const void* W, bool own_unsupported, int M, int N, const float* bias,
                               int act, float dropout_p, unsigned seed, float alpha, const float* R, int ldr, float* outF,
                               int ldof, void* outH, int ldoh) {
    if (!A || !W || (!outF && !outH) || M <= 0) return IA_INVALID_VALUE;
    if (own_unsupported || N % 8 != 0 || (R && ldr % 4 != 0) || (outF && ldof % 4 != 0) || (outH && ldoh % 8 != 0)) return IA_UNSUPPORTED;
    if (!ia_is_aligned(A, 16) || !ia_is_aligned(W, 16) || (bias && !ia_is_aligned(bias, 16)) || (R && !ia_is_aligned(R, 16)) ||
        (outF && !ia_is_aligned(outF, 16)) || (outH && !ia_is_aligned(outH, 16)) || dropout_p < 0.f || dropout_p >= 1.f)
        return IA_INVALID_VALUE;
    const ia_dropout_t d = ia_dropout_rule(dropout_p);
    e.bias = bias; e.R = R; e.outF = outF; e.outH = (__bf16*)outH;
    e.M = M; e.N = N; e.ldr = ldr; e.ldof = ldof; e.ldoh = ldoh;
    e.act = act; e.alpha = alpha; e.seed = seed; e.thr = d.thr; e.keep_scale = d.keep_scale;
    return IA_OK;
}

}  // namespace
