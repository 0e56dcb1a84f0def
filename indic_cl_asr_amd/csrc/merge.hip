// Model merging over the flat fp32 parameter buffer: K task vectors tau_k = theta_k - base, rows of ONE [max_tasks, stride] buffer
// laid out as theta (cl.GEM's convention for its reference gradients), combined into theta in one pass.
//   ia_merge_linear   task arithmetic (Ilharco et al., ICLR 2023) and weight averaging: theta = base + scale * sum_k coef_k * tau_k
//   ia_merge_trim     TIES (Yadav et al., NeurIPS 2023), step 1: per (task, scope segment) the magnitude cutoff that keeps the
//                     largest `1 - trim` of the entries, by the exact radix select of ia_pack_prune (csrc/cl_flat.hip) on the
//                     31-bit pattern of |tau|, most significant digit first:
//       merge_hist_kernel   one pass per digit (8, 8, 8 and 7 bits) and task (blockIdx.y).  A workgroup counts the digit of the
//                           elements whose higher digits equal the selector's prefix into a histogram in LDS and adds it to
//                           hist[task][scope][bin] with integer atomics; the LDS histogram is flushed whenever the scope segment
//                           changes, and at the end.  Only elements below a chunk's count are read: never an alignment gap.
//       merge_pick_kernel   one workgroup per (scope segment, task): the first pass fixes n and r = floor(trim * n); every pass
//                           picks the bin that holds the rank, extends the prefix and clears the histogram; the last one
//                           writes the cutoff.
//   ia_merge_ties     steps 2 and 3: elect the sign of the summed surviving entries, average the entries that carry it.
//   ia_merge_fisher   Fisher merging (Matena & Raffel, NeurIPS 2022) in task-vector form: per element the mean of the tau_k weighted
//                     by coef_k * max-by-select(F_k, floor), F_k read from a second row buffer parallel to the task vectors.
//   ia_merge_linear_dare, ia_merge_ties_dare   DARE (Yu et al., ICML 2024): every entry is dropped or divided by keep_prob, by a
//                     counter-based hash of (seed, task, element) (load_row below), before the linear rule or TIES' election.
// Every product, sum and quotient below is rounded to fp32 on its own (contraction off), in task order, so that one torch op
// per rounding reproduces theta and its bf16 image bit for bit.  HBM-streaming kernels: 16-byte accesses in a chunk's body,
// scalar accesses in its tail, grid capped at 2048 workgroups; integer atomics only, so no result depends on scheduling.
#include "ia_common.h"
#include "dropout_mask.h"
#include <type_traits>

namespace {
constexpr int MG_THREADS = 256;
constexpr int MG_MAX = IA_MERGE_MAX_TASKS;
constexpr int MG_BINS = 256, MG_PASSES = 4;
static_assert(MG_BINS == MG_THREADS, "one histogram bin per thread");
static_assert(MG_MAX <= MG_THREADS, "one thread per task loads its cutoff");
__host__ __device__ constexpr int mg_shift(int pass) { return pass == 0 ? 23 : pass == 1 ? 15 : pass == 2 ? 7 : 0; }
__host__ __device__ constexpr int mg_width(int pass) { return pass == 3 ? 7 : 8; }
constexpr unsigned MG_ABS = 0x7FFFFFFFu;

__device__ __forceinline__ unsigned short bf16_bits(float x) {
    __hip_bfloat16 a = __float2bfloat16(x);
    return *reinterpret_cast<unsigned short*>(&a);
}

__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

__device__ __forceinline__ float div_rn(float a, float b) {   // the IEEE-rounded quotient (no reciprocal, no fast division)
#pragma clang fp contract(off)
    return a / b;
}

// W floats (and their bf16 images) moved as one access: W = 4 in a chunk's float4 body (16 bytes), W = 1 in its tail
template <int W>
struct alignas(4 * W) vecf {
    float a[W];
    __device__ __forceinline__ float& operator[](int j) { return a[j]; }
    __device__ __forceinline__ float operator[](int j) const { return a[j]; }
};
template <int W>
struct alignas(2 * W) vech {
    unsigned short a[W];
};
template <int W> __device__ __forceinline__ vecf<W> ldv(const float* p, int64_t at) { return *reinterpret_cast<const vecf<W>*>(p + at); }
template <int W> __device__ __forceinline__ void stv(float* p, int64_t at, const vecf<W>& x) { *reinterpret_cast<vecf<W>*>(p + at) = x; }

// theta = base + scale * m and its bf16 image, the common end of both merges
template <int W>
__device__ __forceinline__ void store_merged(float* __restrict__ theta, const float* __restrict__ base, int64_t at, const vecf<W>& m,
                                             float scale, unsigned short* __restrict__ shadow) {
    const vecf<W> B = ldv<W>(base, at);
    vecf<W> P;
    vech<W> H;
#pragma unroll
    for (int j = 0; j < W; ++j) {
        P[j] = add_rn(B[j], mul_rn(scale, m[j]));
        H.a[j] = bf16_bits(P[j]);
    }
    stv<W>(theta, at, P);
    if (shadow) *reinterpret_cast<vech<W>*>(shadow + at) = H;
}

struct merge_coefs { float c[MG_MAX]; };      // by value in the kernel arguments: no staging buffer, no copy

// ---- DARE: drop and rescale.  Entry i (its index in the flat buffer) of task k (its position in the merge's list) becomes
//   t = keep(seed, k, i) ? tau / keep_prob : +0        (the IEEE-rounded quotient; keep_prob = 1 leaves a kept tau as it is)
//   keep(seed, k, i) = h < keep_threshold,   h = ia_dm_hash32((uint32)i * 0x9E3779B1 + key_k),
//   key_k = ia_dm_hash32(ia_dm_hash32(seed) ^ (k + 1))
// in 32-bit unsigned arithmetic: a 32-bit compare, so that a keep probability of 2^-32 .. 1 - 2^-32 is expressible.  No mask is
// stored: it is a pure function of (seed, k, i), the same on every rank and in every launch.  An entry whose h equals 2^32 - 1
// is dropped under every threshold, also under keep_threshold = 2^32 - 1 (a density of 1): one in 2^32, not special-cased.
struct dare_rule {
    unsigned seed, threshold;
    float keep_prob;
};
struct no_dare {};

__device__ __forceinline__ unsigned dare_key(const dare_rule& d, int k) { return ia_dm_hash32(ia_dm_hash32(d.seed) ^ (unsigned)(k + 1)); }

// row k at `at`, as the rule that follows reads it
template <int W>
__device__ __forceinline__ vecf<W> load_row(const float* __restrict__ vectors, int64_t stride, int k, int64_t at, const no_dare&) {
    return ldv<W>(vectors + (int64_t)k * stride, at);
}
template <int W>
__device__ __forceinline__ vecf<W> load_row(const float* __restrict__ vectors, int64_t stride, int k, int64_t at, const dare_rule& d) {
    vecf<W> T = ldv<W>(vectors + (int64_t)k * stride, at);
    const unsigned key = dare_key(d, k), i0 = (unsigned)at;
#pragma unroll
    for (int j = 0; j < W; ++j) {
        const unsigned h = ia_dm_hash32((i0 + (unsigned)j) * 0x9E3779B1u + key);
        T[j] = h < d.threshold ? div_rn(T[j], d.keep_prob) : 0.f;
    }
    return T;
}

// s = coef_0 * t_0, then s = s + coef_k * t_k for k = 1 .. K-1
template <int W, class Rows>
__device__ __forceinline__ void linear_at(float* __restrict__ theta, const float* __restrict__ base,
                                          const float* __restrict__ vectors, int64_t stride, int K, const merge_coefs& coef,
                                          float scale, int64_t at, unsigned short* __restrict__ shadow, const Rows& rows) {
    vecf<W> S;
    {
        const vecf<W> T = load_row<W>(vectors, stride, 0, at, rows);
#pragma unroll
        for (int j = 0; j < W; ++j) S[j] = mul_rn(coef.c[0], T[j]);
    }
#pragma unroll 4
    for (int k = 1; k < K; ++k) {
        const vecf<W> T = load_row<W>(vectors, stride, k, at, rows);
        const float ck = coef.c[k];
#pragma unroll
        for (int j = 0; j < W; ++j) S[j] = add_rn(S[j], mul_rn(ck, T[j]));
    }
    store_merged<W>(theta, base, at, S, scale, shadow);
}

template <class Rows>
__global__ __launch_bounds__(MG_THREADS) void merge_linear_kernel(float* __restrict__ theta, const float* __restrict__ base,
                                                                  const float* __restrict__ vectors, int64_t stride, int K,
                                                                  merge_coefs coef, float scale, const int4* __restrict__ table,
                                                                  int nchunks, unsigned short* __restrict__ shadow, Rows rows) {
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int4 e = table[c];  // x = offset (multiple of 4), y = count, z = segment id
        const int off = e.x, cnt = e.y, n4 = cnt >> 2;
        for (int q = threadIdx.x; q < n4; q += MG_THREADS)
            linear_at<4>(theta, base, vectors, stride, K, coef, scale, (int64_t)off + 4 * q, shadow, rows);
        for (int i = (n4 << 2) + threadIdx.x; i < cnt; i += MG_THREADS)
            linear_at<1>(theta, base, vectors, stride, K, coef, scale, (int64_t)off + i, shadow, rows);
    }
}

// per-tensor counts of a chunk: a wave sum, an LDS integer atomic per wave, one global integer atomic per chunk and counter.
// sh_cnt was zeroed before the barrier that precedes the chunk's work; the last barrier lets the next chunk rewrite it.
template <int N>
__device__ __forceinline__ void add_seg_counts(const int (&counts)[N], int* sh_cnt, int* __restrict__ seg_counts, int seg,
                                               int nseg) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        int v = counts[i];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, IA_WAVE);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(sh_cnt + i, v);
    }
    __syncthreads();
    if (threadIdx.x < N && sh_cnt[threadIdx.x] && seg >= 0 && seg < nseg)                     // never outside seg_counts
        atomicAdd(seg_counts + N * (int64_t)seg + threadIdx.x, sh_cnt[threadIdx.x]);
    __syncthreads();
}

// ---- Fisher merging.  Per element, in task order, with F_k the importance of task k:
//   g_k = F_k > floor ? F_k : floor       (a select: a NaN or negative importance becomes the floor)
//   a_k = coef_k * g_k
//   num = a_0 * tau_0;  num = num + a_k * tau_k;     den = a_0;  den = den + a_k
//   m   = den > 0 ? num / den : +0
// counts: {elements where no F_k exceeded the floor (a plain coef-weighted mean), elements with den == 0 (the base value)}.
template <int W>
__device__ __forceinline__ void fisher_at(float* __restrict__ theta, const float* __restrict__ base,
                                          const float* __restrict__ vectors, const float* __restrict__ importances,
                                          int64_t stride, int K, const merge_coefs& coef, float floor_, float scale, int64_t at,
                                          unsigned short* __restrict__ shadow, int (&counts)[2]) {
    vecf<W> num, den;
    bool floored[W];
#pragma unroll
    for (int j = 0; j < W; ++j) { num[j] = den[j] = 0.f; floored[j] = true; }
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
        const vecf<W> T = ldv<W>(vectors + (int64_t)k * stride, at);
        const vecf<W> F = ldv<W>(importances + (int64_t)k * stride, at);
        const float ck = coef.c[k];
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const bool above = F[j] > floor_;
            const float a = mul_rn(ck, above ? F[j] : floor_);
            const float p = mul_rn(a, T[j]);
            num[j] = k == 0 ? p : add_rn(num[j], p);
            den[j] = k == 0 ? a : add_rn(den[j], a);
            floored[j] = floored[j] && !above;
        }
    }
    vecf<W> m;
#pragma unroll
    for (int j = 0; j < W; ++j) {
        m[j] = den[j] > 0.f ? div_rn(num[j], den[j]) : 0.f;
        counts[0] += floored[j];
        counts[1] += den[j] == 0.f;
    }
    store_merged<W>(theta, base, at, m, scale, shadow);
}

__global__ __launch_bounds__(MG_THREADS) void merge_fisher_kernel(float* __restrict__ theta, const float* __restrict__ base,
                                                                  const float* __restrict__ vectors,
                                                                  const float* __restrict__ importances, int64_t stride, int K,
                                                                  merge_coefs coef, float floor_, float scale,
                                                                  const int4* __restrict__ table, int nchunks,
                                                                  unsigned short* __restrict__ shadow, int* __restrict__ seg_counts,
                                                                  int nseg) {
    __shared__ int sh_cnt[2];
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int4 e = table[c];
        const int off = e.x, cnt = e.y, n4 = cnt >> 2;
        if (threadIdx.x < 2) sh_cnt[threadIdx.x] = 0;
        __syncthreads();
        int counts[2] = {0, 0};
        for (int q = threadIdx.x; q < n4; q += MG_THREADS)
            fisher_at<4>(theta, base, vectors, importances, stride, K, coef, floor_, scale, (int64_t)off + 4 * q, shadow, counts);
        for (int i = (n4 << 2) + threadIdx.x; i < cnt; i += MG_THREADS)
            fisher_at<1>(theta, base, vectors, importances, stride, K, coef, floor_, scale, (int64_t)off + i, shadow, counts);
        add_seg_counts<2>(counts, sh_cnt, seg_counts, e.z, nseg);
    }
}

// ---- trim: the radix select
struct alignas(16) merge_sel {    // per (task, scope segment), in the workspace (zeroed by the host before the first pass)
    unsigned prefix;              // the digits chosen so far, in place; after the last pass the cutoff's pattern
    unsigned rank;                // 1-based rank of the cutoff among the elements that share the prefix
    unsigned r;                   // floor(trim * n); 0: the cutoff is 0, everything stays
    unsigned n;                   // elements of the scope segment
};

__device__ __forceinline__ int scope_of(const int* __restrict__ seg_of_scope, int seg, int nscope) {
    const int s = seg_of_scope[seg];
    return s < 0 ? 0 : (s >= nscope ? nscope - 1 : s);      // selectors and cutoffs are never indexed outside their tables
}

__device__ __forceinline__ void mg_flush(unsigned* sh, unsigned* __restrict__ hist, int scope) {
    __syncthreads();
    const unsigned h = sh[threadIdx.x];
    if (h) atomicAdd(hist + (int64_t)scope * MG_BINS + threadIdx.x, h);
    sh[threadIdx.x] = 0;
    __syncthreads();
}

__global__ __launch_bounds__(MG_THREADS) void merge_hist_kernel(const float* __restrict__ vectors, int64_t stride,
                                                                const int4* __restrict__ table, int nchunks,
                                                                const int* __restrict__ seg_of_scope, int nscope,
                                                                const merge_sel* __restrict__ sel, int pass,
                                                                unsigned* __restrict__ hist) {
    __shared__ unsigned sh[MG_BINS];
    sh[threadIdx.x] = 0;
    __syncthreads();
    const int task = blockIdx.y;
    const float* __restrict__ row = vectors + (int64_t)task * stride;
    sel += (int64_t)task * nscope;
    hist += (int64_t)task * nscope * MG_BINS;
    const int shift = mg_shift(pass), up = shift + mg_width(pass);       // up == 31 in the first pass: every pattern matches
    const unsigned digit_mask = (1u << mg_width(pass)) - 1u;
    int cur = -1;                                                         // the scope segment the LDS histogram belongs to
    unsigned prefix_up = 0;
    bool counted = true;                                                  // false: r == 0, nothing to select here
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int4 e = table[c];
        const int scope = scope_of(seg_of_scope, e.z, nscope);           // workgroup-uniform, as everything up to the counting
        if (scope != cur) {
            if (cur >= 0) mg_flush(sh, hist, cur);
            cur = scope;
            if (pass > 0) {
                const merge_sel s = sel[scope];
                prefix_up = s.prefix >> up;
                counted = s.r != 0;
            }
        }
        if (!counted) continue;
        const int off = e.x, cnt = e.y, n4 = cnt >> 2;
        for (int q = threadIdx.x; q < n4; q += MG_THREADS) {
            const uint4 x = reinterpret_cast<const uint4*>(row + off)[q];
            const unsigned k0 = x.x & MG_ABS, k1 = x.y & MG_ABS, k2 = x.z & MG_ABS, k3 = x.w & MG_ABS;
            if (k0 >> up == prefix_up) atomicAdd(sh + ((k0 >> shift) & digit_mask), 1u);
            if (k1 >> up == prefix_up) atomicAdd(sh + ((k1 >> shift) & digit_mask), 1u);
            if (k2 >> up == prefix_up) atomicAdd(sh + ((k2 >> shift) & digit_mask), 1u);
            if (k3 >> up == prefix_up) atomicAdd(sh + ((k3 >> shift) & digit_mask), 1u);
        }
        for (int i = (n4 << 2) + threadIdx.x; i < cnt; i += MG_THREADS) {
            const unsigned k = __float_as_uint(row[off + i]) & MG_ABS;
            if (k >> up == prefix_up) atomicAdd(sh + ((k >> shift) & digit_mask), 1u);
        }
    }
    if (cur >= 0) mg_flush(sh, hist, cur);
}

__global__ __launch_bounds__(MG_BINS) void merge_pick_kernel(unsigned* __restrict__ hist, merge_sel* __restrict__ sel, int nscope,
                                                             int pass, float trim, unsigned* __restrict__ cutoffs) {
    __shared__ unsigned sc[MG_BINS];
    const int scope = blockIdx.x, task = blockIdx.y, t = threadIdx.x;
    const int64_t at = (int64_t)task * nscope + scope;
    const merge_sel s = sel[at];
    if (pass > 0 && !s.r) return;                                        // workgroup-uniform
    const unsigned h = hist[at * MG_BINS + t];
    hist[at * MG_BINS + t] = 0;                                          // for the next pass
    sc[t] = h;
    __syncthreads();
    for (int d = 1; d < MG_BINS; d <<= 1) {                              // inclusive scan
        const unsigned a = t >= d ? sc[t - d] : 0u;
        __syncthreads();
        sc[t] += a;
        __syncthreads();
    }
    const unsigned incl = sc[t], excl = incl - h;
    unsigned rank = s.rank, r = s.r, n = s.n;
    if (pass == 0) {
        n = sc[MG_BINS - 1];
        rank = r = (unsigned)floor((double)trim * (double)n);            // trim < 1, so r < n
        if (r == 0) {
            if (t == 0) {
                sel[at] = {0u, 0u, 0u, n};
                cutoffs[at] = 0u;                                        // |tau| >= 0: everything stays
            }
            return;
        }
    }
    if (h && excl < rank && rank <= incl) {                              // one thread
        const unsigned prefix = s.prefix | ((unsigned)t << mg_shift(pass));
        sel[at] = {prefix, rank - excl, r, n};
        if (pass == MG_PASSES - 1) cutoffs[at] = prefix;
    }
}

// ---- TIES: elect and merge.  Per element, with t_k = tau_k where |tau_k| >= cutoff (pattern order) and +0 elsewhere (under DARE:
// t_k as load_row leaves it, and no cutoff: the random drop replaces the magnitude trim):
//   mass = t_0 + t_1 + ... in task order;  the elected sign is that of the mass (none when the mass is zero or NaN)
//   m    = (sum of the t_k of that sign, in task order from +0) / (their number), +0 when there is none
// The sums of the positive and of the negative entries are both kept while the rows stream by, so the pass reads every row
// once.  counts: {elements with an entry t_k != 0, elements with entries of both signs, elements whose mass is zero}.
template <int W, class Rows>
__device__ __forceinline__ void ties_at(float* __restrict__ theta, const float* __restrict__ base,
                                        const float* __restrict__ vectors, int64_t stride, int K, const unsigned* sh_cut,
                                        float scale, int64_t at, unsigned short* __restrict__ shadow, int (&counts)[3],
                                        const Rows& rows) {
    constexpr bool trimmed = std::is_same<Rows, no_dare>::value;
    vecf<W> mass, sp, sn;
    int np[W], nn[W];
    bool any[W];
#pragma unroll
    for (int j = 0; j < W; ++j) { mass[j] = sp[j] = sn[j] = 0.f; np[j] = nn[j] = 0; any[j] = false; }
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
        const vecf<W> T = load_row<W>(vectors, stride, k, at, rows);
        const unsigned cut = trimmed ? sh_cut[k] : 0u;
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const float t = (__float_as_uint(T[j]) & MG_ABS) >= cut ? T[j] : 0.f;
            mass[j] = k == 0 ? t : add_rn(mass[j], t);
            const bool pos = t > 0.f, neg = t < 0.f;
            sp[j] = pos ? add_rn(sp[j], t) : sp[j];
            sn[j] = neg ? add_rn(sn[j], t) : sn[j];
            np[j] += pos; nn[j] += neg;
            any[j] = any[j] || t != 0.f;                                 // a NaN entry counts as surviving and carries no sign
        }
    }
    vecf<W> m;
#pragma unroll
    for (int j = 0; j < W; ++j) {
        const bool pos = mass[j] > 0.f, neg = mass[j] < 0.f;
        const int cnt = pos ? np[j] : nn[j];
        m[j] = (pos || neg) && cnt > 0 ? div_rn(pos ? sp[j] : sn[j], (float)cnt) : 0.f;
        counts[0] += any[j];
        counts[1] += np[j] > 0 && nn[j] > 0;
        counts[2] += mass[j] == 0.f;
    }
    store_merged<W>(theta, base, at, m, scale, shadow);
}

// Rows = no_dare: cutoffs [K, nscope] and seg_of_scope are read;  Rows = dare_rule: neither is touched (both may be null)
template <class Rows>
__global__ __launch_bounds__(MG_THREADS) void merge_ties_kernel(float* __restrict__ theta, const float* __restrict__ base,
                                                                const float* __restrict__ vectors, int64_t stride, int K,
                                                                const unsigned* __restrict__ cutoffs,
                                                                const int* __restrict__ seg_of_scope, int nscope, float scale,
                                                                const int4* __restrict__ table, int nchunks,
                                                                unsigned short* __restrict__ shadow, int* __restrict__ seg_counts,
                                                                int nseg, Rows rows) {
    __shared__ unsigned sh_cut[MG_MAX];
    __shared__ int sh_cnt[3];
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int4 e = table[c];
        const int off = e.x, cnt = e.y, n4 = cnt >> 2;
        if constexpr (std::is_same<Rows, no_dare>::value) {
            const int scope = scope_of(seg_of_scope, e.z, nscope);
            if (threadIdx.x < K) sh_cut[threadIdx.x] = cutoffs[(int64_t)threadIdx.x * nscope + scope];
        }
        if (threadIdx.x < 3) sh_cnt[threadIdx.x] = 0;
        __syncthreads();
        int counts[3] = {0, 0, 0};
        for (int q = threadIdx.x; q < n4; q += MG_THREADS)
            ties_at<4>(theta, base, vectors, stride, K, sh_cut, scale, (int64_t)off + 4 * q, shadow, counts, rows);
        for (int i = (n4 << 2) + threadIdx.x; i < cnt; i += MG_THREADS)
            ties_at<1>(theta, base, vectors, stride, K, sh_cut, scale, (int64_t)off + i, shadow, counts, rows);
        add_seg_counts<3>(counts, sh_cnt, seg_counts, e.z, nseg);            // ends with a barrier: the next chunk rewrites sh_cut
    }
}

inline int chunk_grid(int nchunks) { return nchunks < 2048 ? nchunks : 2048; }

inline bool rows_ok(const float* vectors, int64_t stride, int ntasks, const int32_t* chunk_table, int nchunks) {
    return vectors && chunk_table && nchunks > 0 && ntasks >= 1 && ntasks <= MG_MAX && stride > 0 && stride % 4 == 0 &&
           ia_is_aligned(vectors, 16) && ia_is_aligned(chunk_table, 16);
}

inline bool scopes_ok(const int32_t* seg_of_scope, int nscope) {
    return seg_of_scope && nscope > 0 && ia_is_aligned(seg_of_scope, 4);
}

inline bool target_ok(const float* theta, const float* base, float scale, const void* shadow_bf16) {
    return theta && base && isfinite(scale) && ia_is_aligned(theta, 16) && ia_is_aligned(base, 16) &&
           (!shadow_bf16 || ia_is_aligned(shadow_bf16, 8));
}

inline bool counts_ok(const int32_t* seg_counts, int nseg) { return seg_counts && nseg > 0 && ia_is_aligned(seg_counts, 4); }

inline bool dare_ok(float keep_prob) { return keep_prob > 0.f && keep_prob <= 1.f; }           // false for a NaN

inline merge_coefs coefs_of(const float* coef, int ntasks) {             // a host array, read here
    merge_coefs c = {};
    for (int k = 0; k < ntasks; ++k) c.c[k] = coef[k];
    return c;
}

template <class Rows>
int launch_linear(float* theta, const float* base, const float* vectors, int64_t stride, int ntasks, const float* coef, float scale,
                  const int32_t* chunk_table, int nchunks, void* shadow_bf16, ia_stream_t stream, Rows rows) {
    hipLaunchKernelGGL(merge_linear_kernel<Rows>, dim3(chunk_grid(nchunks)), dim3(MG_THREADS), 0, (hipStream_t)stream, theta, base,
                       vectors, stride, ntasks, coefs_of(coef, ntasks), scale, (const int4*)chunk_table, nchunks,
                       (unsigned short*)shadow_bf16, rows);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}

template <class Rows>
int launch_ties(float* theta, const float* base, const float* vectors, int64_t stride, int ntasks, const uint32_t* cutoffs,
                const int32_t* seg_of_scope, int nscope, float scale, const int32_t* chunk_table, int nchunks, int nseg,
                void* shadow_bf16, int32_t* seg_counts, ia_stream_t stream, Rows rows) {
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(seg_counts, 0, (size_t)nseg * 3 * sizeof(int32_t), st) != hipSuccess) return IA_LAUNCH_FAILED;
    hipLaunchKernelGGL(merge_ties_kernel<Rows>, dim3(chunk_grid(nchunks)), dim3(MG_THREADS), 0, st, theta, base, vectors, stride,
                       ntasks, (const unsigned*)cutoffs, seg_of_scope, nscope, scale, (const int4*)chunk_table, nchunks,
                       (unsigned short*)shadow_bf16, seg_counts, nseg, rows);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}
}  // namespace

extern "C" int ia_merge_linear(float* theta, const float* base, const float* vectors, int64_t stride, int ntasks,
                               const float* coef, float scale, const int32_t* chunk_table, int nchunks, void* shadow_bf16,
                               ia_stream_t stream) {
    if (!rows_ok(vectors, stride, ntasks, chunk_table, nchunks) || !target_ok(theta, base, scale, shadow_bf16) || !coef)
        return IA_INVALID_VALUE;
    return launch_linear(theta, base, vectors, stride, ntasks, coef, scale, chunk_table, nchunks, shadow_bf16, stream, no_dare{});
}

extern "C" int ia_merge_linear_dare(float* theta, const float* base, const float* vectors, int64_t stride, int ntasks,
                                    const float* coef, float scale, const int32_t* chunk_table, int nchunks, void* shadow_bf16,
                                    uint32_t seed, uint32_t keep_threshold, float keep_prob, ia_stream_t stream) {
    if (!rows_ok(vectors, stride, ntasks, chunk_table, nchunks) || !target_ok(theta, base, scale, shadow_bf16) || !coef ||
        !dare_ok(keep_prob))
        return IA_INVALID_VALUE;
    return launch_linear(theta, base, vectors, stride, ntasks, coef, scale, chunk_table, nchunks, shadow_bf16, stream,
                         dare_rule{seed, keep_threshold, keep_prob});
}

extern "C" int ia_merge_fisher(float* theta, const float* base, const float* vectors, const float* importances, int64_t stride,
                               int ntasks, const float* coef, float floor, float scale, const int32_t* chunk_table, int nchunks,
                               int nseg, void* shadow_bf16, int32_t* seg_counts, ia_stream_t stream) {
    if (!rows_ok(vectors, stride, ntasks, chunk_table, nchunks) || !target_ok(theta, base, scale, shadow_bf16) || !coef ||
        !importances || !ia_is_aligned(importances, 16) || !(isfinite(floor) && floor >= 0.f) || !counts_ok(seg_counts, nseg))
        return IA_INVALID_VALUE;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(seg_counts, 0, (size_t)nseg * 2 * sizeof(int32_t), st) != hipSuccess) return IA_LAUNCH_FAILED;
    hipLaunchKernelGGL(merge_fisher_kernel, dim3(chunk_grid(nchunks)), dim3(MG_THREADS), 0, st, theta, base, vectors, importances,
                       stride, ntasks, coefs_of(coef, ntasks), floor, scale, (const int4*)chunk_table, nchunks,
                       (unsigned short*)shadow_bf16, seg_counts, nseg);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}

// workspace: merge_sel[ntasks][nscope], then the histograms unsigned[ntasks][nscope][MG_BINS]
extern "C" size_t ia_merge_trim_workspace_bytes(int ntasks, int nscope) {
    if (ntasks < 1 || ntasks > MG_MAX || nscope <= 0) return 0;
    return (size_t)ntasks * (size_t)nscope * (sizeof(merge_sel) + MG_BINS * sizeof(unsigned));
}

extern "C" int ia_merge_trim(const float* vectors, int64_t stride, int ntasks, const int32_t* chunk_table, int nchunks,
                             const int32_t* seg_of_scope, int nscope, float trim, uint32_t* cutoffs, void* workspace,
                             size_t workspace_bytes, ia_stream_t stream) {
    if (!rows_ok(vectors, stride, ntasks, chunk_table, nchunks) || !scopes_ok(seg_of_scope, nscope) || !cutoffs || !workspace ||
        !(trim >= 0.f && trim < 1.f) || !ia_is_aligned(cutoffs, 4) || !ia_is_aligned(workspace, 16))
        return IA_INVALID_VALUE;
    const size_t need = ia_merge_trim_workspace_bytes(ntasks, nscope);
    if (workspace_bytes < need) return IA_WORKSPACE_TOO_SMALL;
    hipStream_t st = (hipStream_t)stream;
    merge_sel* sel = (merge_sel*)workspace;
    unsigned* hist = (unsigned*)(sel + (size_t)ntasks * nscope);
    if (hipMemsetAsync(workspace, 0, need, st) != hipSuccess ||
        hipMemsetAsync(cutoffs, 0, (size_t)ntasks * nscope * sizeof(uint32_t), st) != hipSuccess)
        return IA_LAUNCH_FAILED;
    for (int pass = 0; pass < MG_PASSES; ++pass) {
        hipLaunchKernelGGL(merge_hist_kernel, dim3(chunk_grid(nchunks), ntasks), dim3(MG_THREADS), 0, st, vectors, stride,
                           (const int4*)chunk_table, nchunks, seg_of_scope, nscope, sel, pass, hist);
        hipLaunchKernelGGL(merge_pick_kernel, dim3(nscope, ntasks), dim3(MG_BINS), 0, st, hist, sel, nscope, pass, trim, cutoffs);
    }
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}

extern "C" int ia_merge_ties(float* theta, const float* base, const float* vectors, int64_t stride, int ntasks,
                             const uint32_t* cutoffs, const int32_t* seg_of_scope, int nscope, float scale,
                             const int32_t* chunk_table, int nchunks, int nseg, void* shadow_bf16, int32_t* seg_counts,
                             ia_stream_t stream) {
    if (!rows_ok(vectors, stride, ntasks, chunk_table, nchunks) || !scopes_ok(seg_of_scope, nscope) ||
        !target_ok(theta, base, scale, shadow_bf16) || !cutoffs || !seg_counts || nseg <= 0 || !ia_is_aligned(cutoffs, 4) ||
        !ia_is_aligned(seg_counts, 4))
        return IA_INVALID_VALUE;
    return launch_ties(theta, base, vectors, stride, ntasks, cutoffs, seg_of_scope, nscope, scale, chunk_table, nchunks, nseg,
                       shadow_bf16, seg_counts, stream, no_dare{});
}

extern "C" int ia_merge_ties_dare(float* theta, const float* base, const float* vectors, int64_t stride, int ntasks, float scale,
                                  const int32_t* chunk_table, int nchunks, int nseg, void* shadow_bf16, int32_t* seg_counts,
                                  uint32_t seed, uint32_t keep_threshold, float keep_prob, ia_stream_t stream) {
    if (!rows_ok(vectors, stride, ntasks, chunk_table, nchunks) || !target_ok(theta, base, scale, shadow_bf16) ||
        !counts_ok(seg_counts, nseg) || !dare_ok(keep_prob))
        return IA_INVALID_VALUE;
    return launch_ties(theta, base, vectors, stride, ntasks, nullptr, nullptr, 0, scale, chunk_table, nchunks, nseg, shadow_bf16,
                       seg_counts, stream, dare_rule{seed, keep_threshold, keep_prob});
}
