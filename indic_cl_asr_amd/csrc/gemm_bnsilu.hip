// Second pointwise convolution of the Conformer convolution module with the BatchNorm + SiLU in front of it applied while
// the A tile is staged (gfx950):
//
//     out = alpha * dropout( SiLU( BN(z) )[M,K] @ W[N,K]^T + bias ) + R
//
// (ConformerConvolution.forward: batch_norm -> activation -> pointwise_conv2 -> dropout + the residual add of
// ConformerLayer.forward, A/parts/submodules/conformer_modules.py:354-366,182-186).  z is the fp32 output of the depthwise
// convolution; every workgroup derives the per-channel scale / shift from the batch sums (train mode) or the running
// statistics (eval) exactly as ia_bn_silu does, rounds SiLU(BN(z)) to bf16 on its way into LDS, and runs the same
// 16x16x32 bf16 MFMA loop as csrc/gemm_bf16.hip and the tile epilogue both share (gemm_common.h) -- the result is bit-identical
// to ia_bn_silu followed by ia_gemm_bf16 (same rounding points, same k order, same dropout mask), but the [M,K] bf16 tensor
// between them and one launch per block (>= 5 us of stream time however little it does) are gone.  Train-mode running
// statistics are updated by workgroup 0.  Workgroup = 64 rows x 128 columns, 4 waves (2 x 2), k-tiles of 64, one LDS stage +
// register prefetch.
#include <hip/hip_bf16.h>

#include "gemm_common.h"

namespace {

constexpr int BS_BM = 64, BS_BN = 128, BS_BK = 64;
constexpr int BS_ROWB = GEMM_ROWB;        // LDS bytes per tile row (padded: conflict-free 16-byte fragment reads)
constexpr int BS_THREADS = GEMM_THREADS;
constexpr int BS_MAIN = (BS_BM + BS_BN) * BS_ROWB;          // 27 648 B
constexpr int BS_EPI = gemm_epi_bytes(BS_BM, BS_BN);        // 33 792 B
constexpr int BS_REGION = BS_EPI > BS_MAIN ? BS_EPI : BS_MAIN;

struct BsArgs : GemmEpi {
    const float* z; int ldz;
    const float* bn_sum; const float* bn_sumsq; const long long* fixed; const float* gamma; const float* beta;
    float* rm; float* rv; int64_t* nbt; float momentum, eps; int training; int64_t n_rows;
    const __bf16* W; int ldw, K;
    __bf16* outA; int ldoa;   // optional: SiLU(BN(z)) itself, bf16 [M,K] (kept for a backward), written by the first column tile
};

template <bool KEEP>   // KEEP: also write SiLU(BN(z)) to a.outA (first column tile)
__global__ __launch_bounds__(BS_THREADS, 4) void gemm_bnsilu_kernel(BsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* s_scale = reinterpret_cast<float*>(smem + BS_REGION);
    float* s_shift = s_scale + a.K;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, q = lane >> 4;
    const int wm = wave >> 1, wn = wave & 1;
    // ---- per-channel scale / shift (as bn_silu_kernel, csrc/encoder_ops.hip)
    {
        const float inv_n = 1.f / (float)a.n_rows;
        for (int ch = tid; ch < a.K; ch += BS_THREADS) {
            float mean, var;
            if (a.training) {
                // the batch sums: fp32, or the fixed-point accumulators of ia_glu_dwconv_fixed ([sum | sumsq], 2^-24 units)
                float s1, s2;
                if (a.fixed) {
                    long long f1 = 0, f2 = 0;
#pragma unroll
                    for (int r = 0; r < IA_BN_ACC_COPIES; ++r) { f1 += a.fixed[(size_t)r * 2 * a.K + ch]; f2 += a.fixed[(size_t)r * 2 * a.K + a.K + ch]; }
                    s1 = (float)((double)f1 * (1.0 / 16777216.0)); s2 = (float)((double)f2 * (1.0 / 16777216.0));
                } else {
                    s1 = a.bn_sum[ch]; s2 = a.bn_sumsq[ch];
                }
                ia_bn_batch_stats(s1, s2, inv_n, &mean, &var);
            } else {
                mean = a.rm[ch]; var = a.rv[ch];
            }
            ia_bn_scale_shift(mean, var, a.eps, a.gamma[ch], a.beta[ch], &s_scale[ch], &s_shift[ch]);
            if (a.training && a.rm && a.rv && blockIdx.x == 0) {   // nobody reads the running statistics in this mode
                ia_bn_running_update(&a.rm[ch], &a.rv[ch], mean, var, (float)a.n_rows, a.momentum);
                if (ch == 0 && a.nbt) a.nbt[0] += 1;
            }
        }
    }
    int m0, n0;   // (padding workgroups leave after the running-statistics update of workgroup 0, which is row tile 0)
    if (!gemm_xcd_tile<BS_BM, BS_BN>(a.M, a.N, m0, n0)) return;

    constexpr int WM = BS_BM / 2, WN = BS_BN / 2, TI = WM / 16, TJ = WN / 16;
    f4 acc[TI][TJ];
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j) acc[i][j] = (f4){0.f, 0.f, 0.f, 0.f};

    // ---- staging: A = 64 rows x 64 k fp32 (4 float4 per thread: row (tid + 256 i) >> 4, k-quad (tid & 15)), W = 128 rows x 64 k bf16
    float4 fa[4];
    GemmRegTile<BS_BN> rb;
    const int kq = tid & 15;
    unsigned char* const sw = smem + BS_BM * BS_ROWB;
    const unsigned char* sa = smem + (wm * WM + c) * BS_ROWB + q * 16;
    const unsigned char* sb = sw + (wn * WN + c) * BS_ROWB + q * 16;
    gemm_staged_loop(
        (a.K + BS_BK - 1) / BS_BK,
        [&](int kt) {
            const int kk = kt * BS_BK + kq * 4;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = (tid + i * BS_THREADS) >> 4;
                const int gr = (m0 + row < a.M) ? (m0 + row) : (a.M - 1);
                fa[i] = *reinterpret_cast<const float4*>(a.z + (size_t)gr * a.ldz + (kk < a.K ? kk : 0));   // (zeroed in the store)
            }
            rb.load(a.W, a.ldw, n0, a.N, kt * BS_BK, a.K);
            if (kt == 0) __syncthreads();   // scale / shift visible before the first store (the first tile's loads are in flight)
        },
        [&](int kt) {
            // SiLU(BN(z)) rounded to bf16: four k-consecutive values of one row -> 8 bytes of the A tile
            const int kk = kt * BS_BK + kq * 4;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = (tid + i * BS_THREADS) >> 4;
                union { uint2 u; __bf16 h[4]; } o;
                if (kk < a.K) {
                    const float4 sc = *reinterpret_cast<const float4*>(s_scale + kk);
                    const float4 sh = *reinterpret_cast<const float4*>(s_shift + kk);
                    o.h[0] = (__bf16)ia_bn_silu_value(fa[i].x, sc.x, sh.x); o.h[1] = (__bf16)ia_bn_silu_value(fa[i].y, sc.y, sh.y);
                    o.h[2] = (__bf16)ia_bn_silu_value(fa[i].z, sc.z, sh.z); o.h[3] = (__bf16)ia_bn_silu_value(fa[i].w, sc.w, sh.w);
                } else {
                    o.u = make_uint2(0, 0);
                }
                *reinterpret_cast<uint2*>(smem + row * BS_ROWB + kq * 8) = o.u;
                if (KEEP && n0 == 0 && m0 + row < a.M && kk < a.K)
                    *reinterpret_cast<uint2*>(a.outA + (size_t)(m0 + row) * a.ldoa + kk) = o.u;
            }
            rb.store(sw);
        },
        [&](int) { gemm_mfma_bf16_ktile(sa, sb, acc); });

    gemm_tile_epilogue<BS_BM, BS_BN>(a, acc, smem, m0, n0);   // bias, dropout, alpha, residual, fp32 / bf16 outputs
}

}  // namespace

extern "C" int ia_gemm_bnsilu_supported(int K) { return (K > 0 && K <= 1024 && K % 8 == 0) ? 1 : 0; }

extern "C" int ia_gemm_bnsilu_bf16(const float* z, int ldz, int64_t n_rows, const float* bn_sum, const float* bn_sumsq,
                                   const float* gamma, const float* beta, float* running_mean, float* running_var,
                                   int64_t* num_batches_tracked, float momentum, float eps, int training, const void* W, int ldw,
                                   int M, int N, int K, const float* bias, float dropout_p, unsigned seed, float alpha,
                                   const float* R, int ldr, float* outF, int ldof, void* outH, int ldoh,
                                   const long long* bn_sums_fixed, ia_stream_t stream) {
    return ia_gemm_bnsilu_bf16_keep(z, ldz, n_rows, bn_sum, bn_sumsq, gamma, beta, running_mean, running_var, num_batches_tracked,
                                    momentum, eps, training, W, ldw, M, N, K, bias, dropout_p, seed, alpha, R, ldr, outF, ldof, outH,
                                    ldoh, bn_sums_fixed, nullptr, 0, stream);
}

extern "C" int ia_gemm_bnsilu_bf16_keep(const float* z, int ldz, int64_t n_rows, const float* bn_sum, const float* bn_sumsq,
                                        const float* gamma, const float* beta, float* running_mean, float* running_var,
                                        int64_t* num_batches_tracked, float momentum, float eps, int training, const void* W,
                                        int ldw, int M, int N, int K, const float* bias, float dropout_p, unsigned seed,
                                        float alpha, const float* R, int ldr, float* outF, int ldof, void* outH, int ldoh,
                                        const long long* bn_sums_fixed, void* outA, int ldoa, ia_stream_t stream) {
    if (outA && (ldoa % 4 != 0 || ldoa < K || !ia_is_aligned(outA, 8))) return IA_INVALID_VALUE;
    if (!gamma || !beta || N <= 0 || n_rows <= 0) return IA_INVALID_VALUE;
    if (training ? (!bn_sums_fixed && (!bn_sum || !bn_sumsq)) : (!running_mean || !running_var)) return IA_INVALID_VALUE;
    const bool unsupported = !ia_gemm_bnsilu_supported(K) || ldz % 4 != 0 || ldw % 8 != 0;
    BsArgs a = {};
    if (const int rc = gemm_check_and_fill(a, z, W, unsupported, M, N, bias, 0, dropout_p, seed, alpha, R, ldr, outF, ldof, outH, ldoh)) return rc;
    a.z = z; a.ldz = ldz; a.bn_sum = bn_sum; a.bn_sumsq = bn_sumsq; a.fixed = bn_sums_fixed; a.gamma = gamma; a.beta = beta;
    a.rm = running_mean; a.rv = running_var; a.nbt = num_batches_tracked; a.momentum = momentum; a.eps = eps;
    a.training = training; a.n_rows = n_rows;
    a.W = (const __bf16*)W; a.ldw = ldw; a.K = K; a.outA = (__bf16*)outA; a.ldoa = ldoa;
    const int grid = gemm_xcd_grid(M, N, BS_BM, BS_BN);
    const size_t lds = (size_t)BS_REGION + (size_t)2 * K * sizeof(float);
    if (outA) hipLaunchKernelGGL(gemm_bnsilu_kernel<true>, dim3(grid), dim3(BS_THREADS), lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(gemm_bnsilu_kernel<false>, dim3(grid), dim3(BS_THREADS), lds, (hipStream_t)stream, a);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}
