// LoRA (Hu et al. 2021) on the flat buffers: the network keeps reading theta = base + s * B * A, the existing backward keeps
// producing the full dW, and the optimizer step trains the thin factors.  Per adapted tensor W[m, n] (m = shape[0], n = numel / m)
// the factor buffer holds B [m, r] then A [r, n], row-major, each on a 64-float boundary.
//   ia_lora_grad    G = grad * grad_scale [* coef];  gB = s * (G * A^T),  gA = s * (B^T * G), from the pre-step factors.
//                   lora_grad_kernel: one workgroup per 64 x 256 tile of G.  The tile is read from HBM once (scaled on the way)
//                   into LDS with the matching rows of B and columns of A; a thread reads its column of the tile with 4-byte
//                   loads that the wave coalesces, so rows that are not 16-byte aligned (n % 4 != 0) cost nothing extra.  Then
//                   every thread owns one column of the tile and sums B^T * G over the tile's rows, and one row of a quarter of
//                   the tile and sums G * A^T over its columns.  Both partial products go to the workspace with plain stores:
//                   gA's per row tile, gB's per column tile.  LDS: 66 KB for the tile of G + (256 + 64) * 4 * r' B for the factors
//                   (r' = r rounded up to 8) + 8 KB: 94 KB at r = 16, so one workgroup per CU.
//                   lora_finish_kernel: walks the factor buffer's chunk table, 256 elements per workgroup, and adds the partials of
//                   every element in ascending tile order, times s.  No float atomic anywhere and no order that depends on
//                   scheduling: same inputs, same bits.
//                   Liveness of a factor is its parent's (any non-zero gradient bit, or all_active), set here with an integer OR.
//   ia_lora_apply   theta = base + s * (B * A) on adapted tensors (fma over j = 0..r-1 ascending, then one fma with s) and
//                   shadow = bf16(theta) for every tensor.
// The factor update itself is the shared AdamW walker of cl_flat.hip (ia_adamw_step_segmented_kinds on the factor buffer's table).
#include "ia_common.h"
#include <algorithm>

namespace {
constexpr int LR_THREADS = 256;
constexpr int LR_ROWS = 64, LR_COLS = 256;      // the tile of G one workgroup owns
constexpr int LR_GLD = LR_COLS + 1;             // LDS row stride of the G tile: a column walk and a row walk both hit 32 banks
constexpr int LR_JB = 8;                        // factor columns a thread accumulates at a time
constexpr int LR_SPLIT = 16;                    // workgroups per chunk of the factor table in the finishing pass
constexpr int LR_DESC = 8;                      // int64 per adapted tensor
enum { D_GOFF = 0, D_M, D_N, D_BOFF, D_AOFF, D_WSB, D_WSA, D_SEG };
static_assert(LR_COLS == LR_THREADS && LR_ROWS == 64 && LR_THREADS / 64 == 4, "thread <-> column, lane <-> row");

__device__ __forceinline__ float lr_mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

__device__ __forceinline__ unsigned short lr_bf16_bits(float x) {
    __hip_bfloat16 a = __float2bfloat16(x);
    return *reinterpret_cast<unsigned short*>(&a);
}

__host__ __device__ inline int lr_pad_rank(int rank) { return (rank + LR_JB - 1) / LR_JB * LR_JB; }
inline int64_t lr_row_tiles(int64_t m) { return (m + LR_ROWS - 1) / LR_ROWS; }
inline int64_t lr_col_tiles(int64_t n) { return (n + LR_COLS - 1) / LR_COLS; }
inline size_t lr_lds_bytes(int rank) {
    const int rp = lr_pad_rank(rank);
    return sizeof(float) * ((size_t)LR_ROWS * LR_GLD + (size_t)LR_COLS * rp + (size_t)LR_ROWS * rp + 4 * LR_ROWS * LR_JB);
}

// tensors: int64 [ntensors][8] = {flat offset, m, n, offset of B, offset of A, workspace offset of gB's partials [col tiles][m][r],
// workspace offset of gA's partials [row tiles][r][n], index of the tensor in the flat layout}; offsets in floats.
// tiles: int32 [ntiles][4] = {tensor, row tile, column tile, 0}.
__global__ __launch_bounds__(LR_THREADS) void lora_grad_kernel(const float* __restrict__ grad, const float* __restrict__ factors,
                                                               const int64_t* __restrict__ tensors, const int4* __restrict__ tiles,
                                                               int rank, float grad_scale, const float* __restrict__ norm_state,
                                                               int skip_nonfinite, int all_active, int* __restrict__ factor_active,
                                                               float* __restrict__ ws) {
    extern __shared__ __align__(16) float lds[];
    float coef = 1.f;
    if (norm_state) {
        if (skip_nonfinite && norm_state[2] != 0.f) return;
        coef = norm_state[1];
    }
    const int rp = lr_pad_rank(rank);
    float* Gs = lds;                                  // [LR_ROWS][LR_GLD]
    float* As = Gs + LR_ROWS * LR_GLD;                // [LR_COLS][rp]   A's tile, transposed
    float* Bs = As + LR_COLS * rp;                    // [LR_ROWS][rp]
    float* Ps = Bs + LR_ROWS * rp;                    // [4][LR_ROWS][LR_JB]
    const int tid = threadIdx.x;
    const int4 tile = tiles[blockIdx.x];
    const int64_t* d = tensors + (int64_t)tile.x * LR_DESC;
    const int64_t m = d[D_M], n = d[D_N];
    const int64_t row0 = (int64_t)tile.y * LR_ROWS, col0 = (int64_t)tile.z * LR_COLS;
    const float* __restrict__ G = grad + d[D_GOFF];
    const float* __restrict__ B = factors + d[D_BOFF];
    const float* __restrict__ A = factors + d[D_AOFF];

    // Every load of the tile is issued before the first one is used (the thread's column of G, 64 loads), and the factors'
    // parts in batches of eight behind them; rows past m and columns past n read as +0 and add nothing.
    unsigned nz = 0;
    const bool col_in = col0 + tid < n;
    float g[LR_ROWS];
#pragma unroll
    for (int i = 0; i < LR_ROWS; ++i) g[i] = (col_in && row0 + i < m) ? G[(row0 + i) * n + col0 + tid] : 0.f;
    for (int j0 = 0; j0 < rp; j0 += LR_JB) {
        float a[LR_JB];
#pragma unroll
        for (int u = 0; u < LR_JB; ++u) a[u] = (j0 + u < rank && col_in) ? A[(int64_t)(j0 + u) * n + col0 + tid] : 0.f;
        *reinterpret_cast<float4*>(As + tid * rp + j0) = make_float4(a[0], a[1], a[2], a[3]);
        *reinterpret_cast<float4*>(As + tid * rp + j0 + 4) = make_float4(a[4], a[5], a[6], a[7]);
    }
    for (int idx0 = tid; idx0 < LR_ROWS * rp; idx0 += 4 * LR_THREADS) {
        float b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = idx0 + u * LR_THREADS, i = idx / rp, j = idx - i * rp;
            b[u] = (idx < LR_ROWS * rp && j < rank && row0 + i < m) ? B[(row0 + i) * rank + j] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (idx0 + u * LR_THREADS < LR_ROWS * rp) Bs[idx0 + u * LR_THREADS] = b[u];
    }
#pragma unroll
    for (int i = 0; i < LR_ROWS; ++i) {
        nz |= __float_as_uint(g[i]) & 0x7FFFFFFFu;        // -0.0 counts as zero, as in the liveness pass of the AdamW step
        float x = lr_mul_rn(g[i], grad_scale);
        if (norm_state) x = lr_mul_rn(x, coef);
        Gs[i * LR_GLD + tid] = x;
    }
    // one flag update per workgroup, and only while the flag is still clear: thousands of read-modify-writes of one address
    // would queue up behind each other
    const int any_nz = __syncthreads_or(nz != 0);
    if (tid == 0 && (all_active || any_nz) && __atomic_load_n(factor_active + 2 * tile.x, __ATOMIC_RELAXED) == 0) {
        atomicOr(factor_active + 2 * tile.x, 1);
        atomicOr(factor_active + 2 * tile.x + 1, 1);
    }
    __syncthreads();

    // gA's partial: thread <-> column, the sum over the tile's rows in ascending order
    float* __restrict__ wsA = ws + d[D_WSA] + (int64_t)tile.y * rank * n;
    for (int jb = 0; jb < rp; jb += LR_JB) {
        float acc[LR_JB];
#pragma unroll
        for (int u = 0; u < LR_JB; ++u) acc[u] = 0.f;
#pragma unroll 4
        for (int i = 0; i < LR_ROWS; ++i) {
            const float x = Gs[i * LR_GLD + tid];
            const float4 b0 = *reinterpret_cast<const float4*>(Bs + i * rp + jb);
            const float4 b1 = *reinterpret_cast<const float4*>(Bs + i * rp + jb + 4);
            acc[0] = __builtin_fmaf(b0.x, x, acc[0]); acc[1] = __builtin_fmaf(b0.y, x, acc[1]);
            acc[2] = __builtin_fmaf(b0.z, x, acc[2]); acc[3] = __builtin_fmaf(b0.w, x, acc[3]);
            acc[4] = __builtin_fmaf(b1.x, x, acc[4]); acc[5] = __builtin_fmaf(b1.y, x, acc[5]);
            acc[6] = __builtin_fmaf(b1.z, x, acc[6]); acc[7] = __builtin_fmaf(b1.w, x, acc[7]);
        }
        if (col_in) {
#pragma unroll
            for (int u = 0; u < LR_JB; ++u)
                if (jb + u < rank) wsA[(int64_t)(jb + u) * n + col0 + tid] = acc[u];
        }
    }

    // gB's partial: lane <-> row, wave <-> a quarter of the tile's columns in ascending order; the four quarters are added in order
    float* __restrict__ wsB = ws + d[D_WSB] + (int64_t)tile.z * m * rank;
    const int row = tid & 63, quarter = tid >> 6;
    for (int jb = 0; jb < rp; jb += LR_JB) {
        float acc[LR_JB];
#pragma unroll
        for (int u = 0; u < LR_JB; ++u) acc[u] = 0.f;
        for (int cc = 0; cc < LR_COLS / 4; ++cc) {
            const int c = quarter * (LR_COLS / 4) + cc;
            const float g = Gs[row * LR_GLD + c];
            const float4 a0 = *reinterpret_cast<const float4*>(As + c * rp + jb);
            const float4 a1 = *reinterpret_cast<const float4*>(As + c * rp + jb + 4);
            acc[0] = __builtin_fmaf(g, a0.x, acc[0]); acc[1] = __builtin_fmaf(g, a0.y, acc[1]);
            acc[2] = __builtin_fmaf(g, a0.z, acc[2]); acc[3] = __builtin_fmaf(g, a0.w, acc[3]);
            acc[4] = __builtin_fmaf(g, a1.x, acc[4]); acc[5] = __builtin_fmaf(g, a1.y, acc[5]);
            acc[6] = __builtin_fmaf(g, a1.z, acc[6]); acc[7] = __builtin_fmaf(g, a1.w, acc[7]);
        }
        float* mine = Ps + (quarter * LR_ROWS + row) * LR_JB;
        *reinterpret_cast<float4*>(mine) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        *reinterpret_cast<float4*>(mine + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
        __syncthreads();
        for (int o = tid; o < LR_ROWS * LR_JB; o += LR_THREADS) {
            const int i = o / LR_JB, u = o - i * LR_JB;
            const float sum = ((Ps[o] + Ps[LR_ROWS * LR_JB + o]) + Ps[2 * LR_ROWS * LR_JB + o]) + Ps[3 * LR_ROWS * LR_JB + o];
            if (row0 + i < m && jb + u < rank) wsB[(row0 + i) * rank + jb + u] = sum;
        }
        __syncthreads();
    }
}

// factor_table: the factor buffer's chunk table, int4 = {offset, count, factor (2 t: B of tensor t, 2 t + 1: its A), t}
__global__ __launch_bounds__(LR_THREADS) void lora_finish_kernel(float* __restrict__ factor_grad, const int64_t* __restrict__ tensors,
                                                                 const int4* __restrict__ factor_table, int nfchunks, int rank,
                                                                 float scale, const float* __restrict__ norm_state,
                                                                 int skip_nonfinite, const float* __restrict__ ws) {
    if (norm_state && skip_nonfinite && norm_state[2] != 0.f) return;
    for (int c = blockIdx.x; c < nfchunks * LR_SPLIT; c += gridDim.x) {      // a chunk of 4096 is LR_SPLIT pieces of 256 elements
        const int4 e = factor_table[c / LR_SPLIT];
        const int64_t* d = tensors + (int64_t)e.w * LR_DESC;
        const int64_t m = d[D_M], n = d[D_N];
        const bool is_a = e.z & 1;
        const int64_t numel = is_a ? rank * n : m * rank;
        const int64_t parts = is_a ? (m + LR_ROWS - 1) / LR_ROWS : (n + LR_COLS - 1) / LR_COLS;
        const float* __restrict__ src = ws + (is_a ? d[D_WSA] : d[D_WSB]) + (e.x - (is_a ? d[D_AOFF] : d[D_BOFF]));
        const int i = (c & (LR_SPLIT - 1)) * LR_THREADS + threadIdx.x;
        if (i >= e.y) continue;
        float sum = 0.f;
        for (int64_t t0 = 0; t0 < parts; t0 += 8) {    // eight loads in flight, added in ascending order (+0 past the last)
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = t0 + u < parts ? src[(t0 + u) * numel + i] : 0.f;
#pragma unroll
            for (int u = 0; u < 8; ++u) sum += v[u];
        }
        factor_grad[e.x + i] = lr_mul_rn(scale, sum);
    }
}

// One element of an adapted tensor: base + s * sum_j B[i, j] * A[j, c]
__device__ __forceinline__ float lora_weight(const float* __restrict__ B, const float* __restrict__ A, int64_t n, int rank,
                                             int64_t idx, float base, float scale) {
    const int64_t i = idx / n, c = idx - i * n;
    float acc = 0.f;
    for (int j = 0; j < rank; ++j) acc = __builtin_fmaf(B[i * rank + j], A[(int64_t)j * n + c], acc);
    return __builtin_fmaf(scale, acc, base);
}

// seg_tensor: int32 [nseg], the row of `tensors` of an adapted tensor of the flat layout and -1 for every other one
__global__ __launch_bounds__(LR_THREADS) void lora_apply_kernel(float* __restrict__ p, const float* __restrict__ base,
                                                                const float* __restrict__ factors,
                                                                const int64_t* __restrict__ tensors,
                                                                const int* __restrict__ seg_tensor, const int4* __restrict__ table,
                                                                int nchunks, int rank, float scale,
                                                                unsigned short* __restrict__ shadow_bf16,
                                                                const float* __restrict__ norm_state, int skip_nonfinite) {
    if (norm_state && skip_nonfinite && norm_state[2] != 0.f) return;
    for (int ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        const int4 e = table[ch];
        const int off = e.x, cnt = e.y, n4 = cnt >> 2;
        const int t = seg_tensor[e.z];                 // workgroup-uniform
        if (t < 0) {
            if (shadow_bf16)
                for (int i = threadIdx.x; i < cnt; i += LR_THREADS) shadow_bf16[off + i] = lr_bf16_bits(p[off + i]);
            continue;
        }
        const int64_t* d = tensors + (int64_t)t * LR_DESC;
        const int64_t n = d[D_N], first = off - d[D_GOFF];     // index of the chunk's first element inside the tensor
        const float* __restrict__ B = factors + d[D_BOFF];
        const float* __restrict__ A = factors + d[D_AOFF];
        const bool rows_aligned = (n & 3) == 0;                // then a float4 of theta lies inside one row, 16-byte aligned in A
        for (int q = threadIdx.x; q < n4; q += LR_THREADS) {
            const float4 W0 = reinterpret_cast<const float4*>(base + off)[q];
            const int64_t idx = first + (q << 2);
            float4 P;
            if (rows_aligned) {
                const int64_t i = idx / n, c = idx - i * n;
                float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
                for (int j = 0; j < rank; ++j) {
                    const float b = B[i * rank + j];
                    const float4 a = *reinterpret_cast<const float4*>(A + (int64_t)j * n + c);
                    acc.x = __builtin_fmaf(b, a.x, acc.x); acc.y = __builtin_fmaf(b, a.y, acc.y);
                    acc.z = __builtin_fmaf(b, a.z, acc.z); acc.w = __builtin_fmaf(b, a.w, acc.w);
                }
                P = make_float4(__builtin_fmaf(scale, acc.x, W0.x), __builtin_fmaf(scale, acc.y, W0.y),
                                __builtin_fmaf(scale, acc.z, W0.z), __builtin_fmaf(scale, acc.w, W0.w));
            } else {
                P = make_float4(lora_weight(B, A, n, rank, idx, W0.x, scale), lora_weight(B, A, n, rank, idx + 1, W0.y, scale),
                                lora_weight(B, A, n, rank, idx + 2, W0.z, scale), lora_weight(B, A, n, rank, idx + 3, W0.w, scale));
            }
            reinterpret_cast<float4*>(p + off)[q] = P;
            if (shadow_bf16) {
                ushort4 o;
                o.x = lr_bf16_bits(P.x); o.y = lr_bf16_bits(P.y); o.z = lr_bf16_bits(P.z); o.w = lr_bf16_bits(P.w);
                reinterpret_cast<ushort4*>(shadow_bf16 + off)[q] = o;
            }
        }
        for (int i = (n4 << 2) + threadIdx.x; i < cnt; i += LR_THREADS) {
            const float P = lora_weight(B, A, n, rank, first + i, base[off + i], scale);
            p[off + i] = P;
            if (shadow_bf16) shadow_bf16[off + i] = lr_bf16_bits(P);
        }
    }
}

inline bool rank_ok(int rank) { return rank >= 1 && rank <= IA_LORA_MAX_RANK; }
}  // namespace

extern "C" int ia_lora_tile_rows(void) { return LR_ROWS; }
extern "C" int ia_lora_tile_cols(void) { return LR_COLS; }

extern "C" size_t ia_lora_workspace_bytes(int64_t m, int64_t n, int rank) {
    if (m <= 0 || n <= 0 || !rank_ok(rank)) return 0;
    const size_t floats = (size_t)rank * ((size_t)lr_col_tiles(n) * (size_t)m + (size_t)lr_row_tiles(m) * (size_t)n);
    return ia_align_up(floats * sizeof(float), 256);
}

extern "C" int ia_lora_grad(const float* grad, const float* factors, float* factor_grad, const int64_t* tensors, int ntensors,
                            const int32_t* tiles, int ntiles, const int32_t* factor_chunk_table, int nfchunks, int rank,
                            float scale, float grad_scale, const float* norm_state, int skip_nonfinite, int all_active,
                            int32_t* factor_active, void* workspace, size_t workspace_bytes, size_t workspace_needed,
                            ia_stream_t stream) {
    if (!grad || !factors || !factor_grad || !tensors || !tiles || !factor_chunk_table || !factor_active || !workspace ||
        ntensors <= 0 || ntiles <= 0 || nfchunks <= 0 || !rank_ok(rank))
        return IA_INVALID_VALUE;
    if (!ia_is_aligned(grad, 16) || !ia_is_aligned(factors, 16) || !ia_is_aligned(factor_grad, 16) || !ia_is_aligned(tensors, 8) ||
        !ia_is_aligned(tiles, 16) || !ia_is_aligned(factor_chunk_table, 16) || !ia_is_aligned(factor_active, 4) ||
        !ia_is_aligned(workspace, 16) || (norm_state && !ia_is_aligned(norm_state, 4)))
        return IA_INVALID_VALUE;
    if (workspace_needed == 0 || workspace_bytes < workspace_needed) return IA_WORKSPACE_TOO_SMALL;
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = lr_lds_bytes(rank);
    IA_SET_MAX_LDS_ONCE(lora_grad_kernel, lds);
    hipLaunchKernelGGL(lora_grad_kernel, dim3(ntiles), dim3(LR_THREADS), lds, st, grad, factors, tensors, (const int4*)tiles, rank,
                       grad_scale, norm_state, skip_nonfinite, all_active, factor_active, (float*)workspace);
    hipLaunchKernelGGL(lora_finish_kernel, dim3((int)std::min<int64_t>((int64_t)nfchunks * LR_SPLIT, 8192)), dim3(LR_THREADS), 0, st, factor_grad, tensors,
                       (const int4*)factor_chunk_table, nfchunks, rank, scale, norm_state, skip_nonfinite,
                       (const float*)workspace);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}

extern "C" int ia_lora_apply(float* theta, const float* base, const float* factors, const int64_t* tensors, int ntensors,
                             const int32_t* seg_tensor, const int32_t* chunk_table, int nchunks, int nseg, int rank, float scale,
                             void* shadow_bf16, const float* norm_state, int skip_nonfinite, ia_stream_t stream) {
    if (!theta || !base || !factors || !tensors || !seg_tensor || !chunk_table || ntensors <= 0 || nchunks <= 0 || nseg <= 0 ||
        !rank_ok(rank))
        return IA_INVALID_VALUE;
    if (!ia_is_aligned(theta, 16) || !ia_is_aligned(base, 16) || !ia_is_aligned(factors, 16) || !ia_is_aligned(tensors, 8) ||
        !ia_is_aligned(seg_tensor, 4) || !ia_is_aligned(chunk_table, 16) || (shadow_bf16 && !ia_is_aligned(shadow_bf16, 8)) ||
        (norm_state && !ia_is_aligned(norm_state, 4)))
        return IA_INVALID_VALUE;
    hipLaunchKernelGGL(lora_apply_kernel, dim3(nchunks < 2048 ? nchunks : 2048), dim3(LR_THREADS), 0, (hipStream_t)stream, theta,
                       base, factors, tensors, seg_tensor, (const int4*)chunk_table, nchunks, rank, scale,
                       (unsigned short*)shadow_bf16, norm_state, skip_nonfinite);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}
