// fp8 (OCP e4m3) projection GEMM with per-row scales for the frozen Conformer prefix (gfx950, v_mfma_f32_16x16x32_fp8_fp8):
//
//   out = alpha * dropout(act( (Aq[M,K] @ Wq[N,K]^T) o sa[M] o sw[N] + bias )) + R
//
// Aq / Wq are e4m3 with one f32 scale per row (x ~ scale * q, scale = amax / 448), produced by ia_quantize_fp8_rows --
// weights once per parameter version, activations per call.  BASELINE configs[4] names "fp8 MFMA" for the Conformer-large
// projections; the reference itself has no fp8 semantics, parity is defined against the fp32 oracle with
// the tolerance stated in tests/test_fp8_gpu.py.  Same operator as csrc/gemm_bf16.hip (epilogue, dropout mask and tile
// order are the same code: gemm_common.h): nn.Linear + the elementwise ops around it in ConformerFeedForward
// (A/parts/submodules/conformer_modules.py:385-404), the Q/K/V/out projections (multi_head_attention.py:69-96,117-119)
// and the pointwise convolutions (:340-366).
//
// Workgroup = 4 waves (2 x 2), tile 128 x 128 x 128 (k-tile = 128 bytes per row, 144-byte padded LDS rows: conflict-free
// ds_read_b64 fragments), one LDS stage with the next k-tile prefetched in registers.  The product is computed transposed
// (A operand = weight rows, B operand = activation rows) so that a lane owns 4 consecutive output columns of one row.
#include <hip/hip_bf16.h>

#include "gemm_common.h"

namespace {

constexpr int F8_BM = GEMM_T_BM, F8_BN = GEMM_T_BN, F8_BK = 128;
constexpr int F8_ROWB = GEMM_ROWB;
constexpr int F8_STAGE = (F8_BM + F8_BN) * F8_ROWB;          // 36 864 B
constexpr int F8_LDS = F8_STAGE > GEMM_T_EPI ? F8_STAGE : GEMM_T_EPI;
constexpr float F8_MAX = 448.f;

struct F8Args : GemmEpi {
    const unsigned char* A; const unsigned char* W; const float* sa; const float* sw;
    int K, lda, ldw;
};

__global__ __launch_bounds__(GEMM_THREADS, 2) void gemm_fp8_nt_kernel(F8Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, q = lane >> 4;
    const int wm = wave >> 1, wn = wave & 1;
    int m0, n0;
    if (!gemm_xcd_tile<F8_BM, F8_BN>(a.M, a.N, m0, n0)) return;

    GemmRegTile<F8_BM> ra;   // (bytes >= K read as zero, K % 16 == 0)
    GemmRegTile<F8_BN> rb;
    f4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f4){0.f, 0.f, 0.f, 0.f};

    unsigned char* const sw = smem + F8_BM * F8_ROWB;
    const unsigned char* sa_ = smem + (wm * 64 + c) * F8_ROWB + q * 8;
    const unsigned char* sb_ = sw + (wn * 64 + c) * F8_ROWB + q * 8;
    gemm_staged_loop(
        (a.K + F8_BK - 1) / F8_BK,
        [&](int kt) { ra.load(a.A, a.lda, m0, a.M, kt * F8_BK, a.K); rb.load(a.W, a.ldw, n0, a.N, kt * F8_BK, a.K); },
        [&](int) { ra.store(smem); rb.store(sw); },
        [&](int) {
#pragma unroll
            for (int ks = 0; ks < F8_BK / 32; ++ks) {
                long af[4], wf[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) af[i] = *reinterpret_cast<const long*>(sa_ + i * 16 * F8_ROWB + ks * 32);
#pragma unroll
                for (int j = 0; j < 4; ++j) wf[j] = *reinterpret_cast<const long*>(sb_ + j * 16 * F8_ROWB + ks * 32);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)   // transposed product: rows of the MFMA result = output columns
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(wf[j], af[i], acc[i][j], 0, 0, 0);
            }
        });
    gemm_tile_epilogue_t<true>(a, acc, smem, m0, n0, a.sa, a.sw);
}

// one wave per row: amax, scale = amax / 448 (1 for an all-zero row), q = e4m3(x / scale).  K % 8 == 0, rows 16-byte aligned.
template <bool F32>
__global__ __launch_bounds__(256) void quantize_fp8_rows_kernel(const void* __restrict__ x, int ld, int64_t M, int K,
                                                                unsigned char* __restrict__ qout, int ldq, float* __restrict__ scale) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int nv = K / 8;
    float amax = 0.f;
    for (int v = lane; v < nv; v += 64) {
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
#pragma unroll
        for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(e[j]));
    }
    amax = ia_wave_max_dpp(amax);   // wave-uniform
    const float s = amax > 0.f ? amax / F8_MAX : 1.f;
    const float inv = 1.f / s;
    if (lane == 0) scale[row] = s;
    for (int v = lane; v < nv; v += 64) {
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
        int w0 = 0, w1 = 0;
        w0 = __builtin_amdgcn_cvt_pk_fp8_f32(e[0] * inv, e[1] * inv, w0, false);
        w0 = __builtin_amdgcn_cvt_pk_fp8_f32(e[2] * inv, e[3] * inv, w0, true);
        w1 = __builtin_amdgcn_cvt_pk_fp8_f32(e[4] * inv, e[5] * inv, w1, false);
        w1 = __builtin_amdgcn_cvt_pk_fp8_f32(e[6] * inv, e[7] * inv, w1, true);
        *reinterpret_cast<int2*>(qout + row * ldq + v * 8) = make_int2(w0, w1);
    }
    // zero the padding bytes K .. ldq (ldq = K rounded up to 16)
    for (int k = K + lane; k < ldq; k += 64) qout[row * ldq + k] = 0;
}

}  // namespace

extern "C" int ia_quantize_fp8_rows(const void* x, int is_f32, int ld, int64_t M, int K, void* q, int ldq, float* scale,
                                    ia_stream_t stream) {
    if (!x || !q || !scale || M <= 0 || K <= 0 || K % 8 != 0 || ld < K || ldq < K || ldq % 16 != 0) return IA_INVALID_VALUE;
    if ((is_f32 ? ld % 4 : ld % 8) != 0 || !ia_is_aligned(x, 16) || !ia_is_aligned(q, 16)) return IA_INVALID_VALUE;
    const unsigned grid = (unsigned)((M + 3) / 4);
    if (is_f32)
        hipLaunchKernelGGL(quantize_fp8_rows_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, ld, M, K,
                           (unsigned char*)q, ldq, scale);
    else
        hipLaunchKernelGGL(quantize_fp8_rows_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, ld, M, K,
                           (unsigned char*)q, ldq, scale);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}

extern "C" int ia_gemm_fp8(const void* Aq, int lda, const float* a_scale, const void* Wq, int ldw, const float* w_scale, int M,
                           int N, int K, const float* bias, int act, float dropout_p, unsigned seed, float alpha,
                           const float* R, int ldr, float* outF, int ldof, void* outH, int ldoh, ia_stream_t stream) {
    if (!a_scale || !w_scale || N <= 0 || K <= 0) return IA_INVALID_VALUE;
    const bool unsupported = K % 16 != 0 || lda % 16 != 0 || ldw % 16 != 0;
    F8Args a = {};
    if (const int rc = gemm_check_and_fill(a, Aq, Wq, unsupported, M, N, bias, act, dropout_p, seed, alpha, R, ldr, outF, ldof, outH, ldoh)) return rc;
    if (!ia_is_aligned(w_scale, 16) || act < 0 || act > 2) return IA_INVALID_VALUE;
    a.A = (const unsigned char*)Aq; a.W = (const unsigned char*)Wq; a.sa = a_scale; a.sw = w_scale; a.K = K; a.lda = lda; a.ldw = ldw;
    hipLaunchKernelGGL(gemm_fp8_nt_kernel, dim3(gemm_xcd_grid(M, N, F8_BM, F8_BN)), dim3(GEMM_THREADS), F8_LDS, (hipStream_t)stream, a);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}
