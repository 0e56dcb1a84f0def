// Block-scaled fp8 (MX: OCP e4m3 elements, one e8m0 scale per 32 consecutive k) projection GEMM on gfx950's
// v_mfma_scale_f32_16x16x128_f8f6f4 -- the instruction that issues fp8 at TWICE the bf16 rate (the non-scaled
// v_mfma_f32_16x16x32_fp8_fp8 of csrc/gemm_fp8.hip runs at the bf16 rate: MI355X_MICROARCH.md, MFMA table):
//
//   out = alpha * dropout(act( (A o 2^sa)[M,K] @ (W o 2^sw)[N,K]^T + bias )) + R
//
// BASELINE configs[4] names "fp8 MFMA" for the Conformer-large projections; same operator as csrc/gemm_bf16.hip
// (A/parts/submodules/conformer_modules.py:340-404, multi_head_attention.py:69-119), epilogue and tile order are gemm_common.h's.
//
// Operand maps of the instruction, found with exact integer data (tools/probe_mfma_scale.hip, probe_mfma_scale2.hip; the
// programming guide gives the C/D map only):
//   data   lane l = (row r = l & 15, group kg = l >> 4) supplies 32 bytes; its register half h (16 bytes) holds
//          k = 64 (kg >> 1) + 32 h + 16 (kg & 1) + j, j = 0..15           (for A: row r of A; for B: column r of B)
//   scale  byte [opsel] of the scale register of lane 16 sg + r is the e8m0 scale of the 32-block Bk = 2 (sg & 1) + (sg >> 1)
//          of that row / column (so each lane shifts its row's 4-byte scale word by 8 Bk)
//   C / D  the shape's standard map (col = l & 15, row = 4 (l >> 4) + reg)
// Workgroup = 4 waves (2 x 2), tile 128 x 128 x 128 bytes of k per step = ONE scaled MFMA per 16 x 16 output tile and step,
// 144-byte padded LDS rows (conflict-free 16-byte fragment reads), one LDS stage with the next k-tile prefetched in
// registers; the product is computed transposed (A operand = weight rows) so that a lane owns 4 consecutive output columns.
#include <hip/hip_bf16.h>

#include "gemm_common.h"

namespace {

typedef int v8i __attribute__((ext_vector_type(8)));

constexpr int MX_BM = GEMM_T_BM, MX_BN = GEMM_T_BN, MX_BK = 128;
constexpr int MX_ROWB = GEMM_ROWB;
constexpr int MX_STAGE = (MX_BM + MX_BN) * MX_ROWB;
constexpr int MX_LDS = MX_STAGE > GEMM_T_EPI ? MX_STAGE : GEMM_T_EPI;

struct MxArgs : GemmEpi {
    const unsigned char* A; const unsigned char* W; const unsigned char* sa; const unsigned char* sw;
    int K, lda, ldw, ldsa, ldsw;
};

__global__ __launch_bounds__(GEMM_THREADS, 2) void gemm_mxfp8_nt_kernel(MxArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, kg = lane >> 4;
    const int wm = wave >> 1, wn = wave & 1;
    int m0, n0;
    if (!gemm_xcd_tile<MX_BM, MX_BN>(a.M, a.N, m0, n0)) return;
    const int bsh = 8 * (2 * (kg & 1) + (kg >> 1));           // this lane's 32-block inside a k-tile -> byte of the scale word

    GemmRegTile<MX_BM, false> ra;   // (K % 128 == 0: whole k-tiles)
    GemmRegTile<MX_BN, false> rb;
    // scale words (4 e8m0 bytes = the 4 blocks of one k-tile) of this lane's 4 + 4 fragment rows: byte offsets of the rows, the
    // prefetched k-tile's words and the staged k-tile's bytes
    unsigned sa_off[4], sw_off[4], nxt_a[4], nxt_w[4], cur_a[4], cur_w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int gm = m0 + wm * 64 + i * 16 + c; gm = gm < a.M ? gm : a.M - 1;
        int gn = n0 + wn * 64 + i * 16 + c; gn = gn < a.N ? gn : a.N - 1;
        sa_off[i] = (unsigned)gm * (unsigned)a.ldsa;
        sw_off[i] = (unsigned)gn * (unsigned)a.ldsw;
    }
    // the prefetched words become the current bytes behind a k-tile's MFMAs, never in the store: the words are the last loads a
    // k-step issues, and the LDS stores must wait for the tile loads only
    auto take_scales = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) { cur_a[i] = (nxt_a[i] >> bsh) & 0xFFu; cur_w[i] = (nxt_w[i] >> bsh) & 0xFFu; }
    };
    f4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f4){0.f, 0.f, 0.f, 0.f};

    const int koff = 64 * (kg >> 1) + 16 * (kg & 1);
    unsigned char* const sw = smem + MX_BM * MX_ROWB;
    const unsigned char* sa_ = smem + (wm * 64 + c) * MX_ROWB + koff;
    const unsigned char* sb_ = sw + (wn * 64 + c) * MX_ROWB + koff;
    gemm_staged_loop(
        a.K / MX_BK,
        [&](int kt) {
            ra.load(a.A, a.lda, m0, a.M, kt * MX_BK, a.K);
            rb.load(a.W, a.ldw, n0, a.N, kt * MX_BK, a.K);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                nxt_a[i] = *reinterpret_cast<const unsigned*>(a.sa + sa_off[i] + 4 * kt);
                nxt_w[i] = *reinterpret_cast<const unsigned*>(a.sw + sw_off[i] + 4 * kt);
            }
            if (kt == 0) take_scales();
        },
        [&](int) { ra.store(smem); rb.store(sw); },
        [&](int) {
            v8i af[4], wf[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint4 lo = *reinterpret_cast<const uint4*>(sa_ + i * 16 * MX_ROWB), hi = *reinterpret_cast<const uint4*>(sa_ + i * 16 * MX_ROWB + 32);
                af[i] = (v8i){(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
                const uint4 wl = *reinterpret_cast<const uint4*>(sb_ + i * 16 * MX_ROWB), wh = *reinterpret_cast<const uint4*>(sb_ + i * 16 * MX_ROWB + 32);
                wf[i] = (v8i){(int)wl.x, (int)wl.y, (int)wl.z, (int)wl.w, (int)wh.x, (int)wh.y, (int)wh.z, (int)wh.w};
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)   // transposed product: the MFMA's rows = output columns (weight rows), columns = activation rows
                    acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[j], af[i], acc[i][j], 0, 0, 0, (int)cur_w[j], 0, (int)cur_a[i]);
            take_scales();   // the prefetched k-tile's, if there is one
        });
    gemm_tile_epilogue_t<false>(a, acc, smem, m0, n0);   // (no operand scales left to apply)
}

// MX quantiser: per 32 consecutive k of a row, e = smallest exponent with amax / 2^e <= 448 (ilogb(amax) - 8, + 1 if that
// still exceeds 448), scale byte = e + 127 (e8m0), q = e4m3(x / 2^e).  Thread = 8 elements; a block = 4 adjacent lanes.
template <bool F32>
__global__ __launch_bounds__(256) void quantize_mxfp8_kernel(const void* __restrict__ x, int ld, int64_t M, int K,
                                                             unsigned char* __restrict__ q, int ldq,
                                                             unsigned char* __restrict__ scales, int lds) {
    const int nv = K / 8;
    const int64_t total = M * nv;
    for (int64_t i0 = (int64_t)blockIdx.x * 256; i0 < total; i0 += (int64_t)gridDim.x * 256) {
        const int64_t i = i0 + threadIdx.x;
        const bool live = i < total;
        const int64_t row = live ? i / nv : 0;
        const int v = live ? (int)(i - row * nv) : 0;
        float e[8];
        if (F32) {
            const float4 a0 = *reinterpret_cast<const float4*>((const float*)x + row * ld + v * 8);
            const float4 a1 = *reinterpret_cast<const float4*>((const float*)x + row * ld + v * 8 + 4);
            e[0] = a0.x; e[1] = a0.y; e[2] = a0.z; e[3] = a0.w; e[4] = a1.x; e[5] = a1.y; e[6] = a1.z; e[7] = a1.w;
        } else {
            union { uint4 u; __bf16 h[8]; } a;
            a.u = *reinterpret_cast<const uint4*>((const __bf16*)x + row * ld + v * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) e[j] = (float)a.h[j];
        }
        float amax = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(e[j]));
        if (!live) amax = 0.f;
        amax = fmaxf(amax, __shfl_xor(amax, 1, 64));   // nv % 4 == 0: the 4 lanes of a block are adjacent and in one row
        amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
        int ex = 0;
        if (amax > 0.f) {
            ex = ilogbf(amax) - 8;
            if (ldexpf(amax, -ex) > 448.f) ++ex;
            ex = ex < -127 ? -127 : (ex > 127 ? 127 : ex);
        }
        const float inv = ldexpf(1.f, -ex);
        if (live) {
            int w0 = 0, w1 = 0;
            w0 = __builtin_amdgcn_cvt_pk_fp8_f32(e[0] * inv, e[1] * inv, w0, false);
            w0 = __builtin_amdgcn_cvt_pk_fp8_f32(e[2] * inv, e[3] * inv, w0, true);
            w1 = __builtin_amdgcn_cvt_pk_fp8_f32(e[4] * inv, e[5] * inv, w1, false);
            w1 = __builtin_amdgcn_cvt_pk_fp8_f32(e[6] * inv, e[7] * inv, w1, true);
            *reinterpret_cast<int2*>(q + row * ldq + v * 8) = make_int2(w0, w1);
            if ((v & 3) == 0) scales[row * lds + (v >> 2)] = (unsigned char)(ex + 127);
        }
    }
}

}  // namespace

extern "C" int ia_quantize_mxfp8(const void* x, int is_f32, int ld, int64_t M, int K, void* q, int ldq, void* scales, int lds,
                                 ia_stream_t stream) {
    if (!x || !q || !scales || M <= 0 || K <= 0 || K % 32 != 0 || ld < K || ldq < K || ldq % 16 != 0 || lds < K / 32 || lds % 4 != 0)
        return IA_INVALID_VALUE;
    if ((is_f32 ? ld % 4 : ld % 8) != 0 || !ia_is_aligned(x, 16) || !ia_is_aligned(q, 16) || !ia_is_aligned(scales, 4)) return IA_INVALID_VALUE;
    const int64_t items = M * (K / 8), blocks = (items + 255) / 256;
    const unsigned grid = (unsigned)(blocks < 16384 ? blocks : 16384);
    if (is_f32)
        hipLaunchKernelGGL(quantize_mxfp8_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, ld, M, K, (unsigned char*)q,
                           ldq, (unsigned char*)scales, lds);
    else
        hipLaunchKernelGGL(quantize_mxfp8_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, ld, M, K, (unsigned char*)q,
                           ldq, (unsigned char*)scales, lds);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}

extern "C" int ia_gemm_mxfp8(const void* Aq, int lda, const void* a_scales, int ldsa, const void* Wq, int ldw, const void* w_scales,
                             int ldsw, int M, int N, int K, const float* bias, int act, float dropout_p, unsigned seed, float alpha,
                             const float* R, int ldr, float* outF, int ldof, void* outH, int ldoh, ia_stream_t stream) {
    if (!a_scales || !w_scales || N <= 0 || K <= 0) return IA_INVALID_VALUE;
    const bool unsupported = K % MX_BK != 0 || lda % 16 != 0 || ldw % 16 != 0 || ldsa % 4 != 0 || ldsw % 4 != 0 || ldsa < K / 32 || ldsw < K / 32;
    MxArgs a = {};
    if (const int rc = gemm_check_and_fill(a, Aq, Wq, unsupported, M, N, bias, act, dropout_p, seed, alpha, R, ldr, outF, ldof, outH, ldoh)) return rc;
    if (!ia_is_aligned(a_scales, 4) || !ia_is_aligned(w_scales, 4) || act < 0 || act > 2) return IA_INVALID_VALUE;
    a.A = (const unsigned char*)Aq; a.W = (const unsigned char*)Wq; a.sa = (const unsigned char*)a_scales; a.sw = (const unsigned char*)w_scales;
    a.K = K; a.lda = lda; a.ldw = ldw; a.ldsa = ldsa; a.ldsw = ldsw;
    hipLaunchKernelGGL(gemm_mxfp8_nt_kernel, dim3(gemm_xcd_grid(M, N, MX_BM, MX_BN)), dim3(GEMM_THREADS), MX_LDS, (hipStream_t)stream, a);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}
