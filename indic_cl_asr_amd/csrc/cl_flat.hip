// Continual-learning regulariser + optimizer kernels over ONE flat fp32 buffer of all trainable parameters
// (the reference launches one set of elementwise kernels per tensor, ~300 per step: SURVEY.md §8 a17/a18/a20).
//   ia_cl_penalty ............ R/cl_baseline_ewc.py:69-81 (2*lambda*F*(theta-theta*), mean_k mean|.| monitor) and
//                              R/cl_baseline_mas.py:70-75 (sum omega*(theta-theta*)^2 and its gradient)
//   ia_cl_fisher_accumulate .. R/cl_baseline_ewc.py:245-255  F += mean(loss) * g^2
//   ia_cl_abs_accumulate ..... R/cl_baseline_mas.py:267-270  omega += |g|
//   ia_adamw_step ............ torch.optim.AdamW single-tensor update (R/cl_baseline.py:137 defaults)
//   ia_si_consolidate ........ end of a task: omega += max(0, w / ((theta-theta*)^2 + xi)), w = 0, theta* = theta
//   ia_rwalk_consolidate ..... end of a language: last fold, device-side maxima, importance = F / max F + mean of score / max score
//   ia_mask_pack, ia_mask_apply .. Piggyback's scores as one bit per weight, and the bits back to weights
//
// The per-tensor ("segmented") AdamW step, ia_adamw_step_segmented*, is ONE kernel, ONE update rule and ONE host routine:
//   adamw_seg_kernel<CLIP, Variant>   the chunk walker.  It owns the skip on a non-finite norm, the chunk loop, the refresh of
//                              the bf16 image of a tensor that is dead (no gradient) or frozen, the group lookup, the fp64
//                              bias-correction constants, the float4 body / scalar tail split and the stores of theta, the
//                              moments and the bf16 image.
//   adamw1_rn<TAIL>            the arithmetic of one element, every rounding written out.
//   a variant                  a small struct passed by value: its extra operands and its rule for one access of W elements
//                              (W = 4 in the body, 1 in the tail).  A rule forms the gradient AdamW consumes, calls adamw1_rn and
//                              loads / stores what is its own:
//       plain_step             consumed_step<scaled_grad>: g * grad_scale [* coef]           ia_adamw_step_segmented[_clipped]
//       si_step<PEN>           Synaptic Intelligence: [+ 2c*omega*(theta-theta*)] after the clip, and the path integral
//                              w -= ge * (theta' - theta)                                     ia_adamw_step_segmented_si
//       rwalk_step<PEN, SCORES, FOLD>   Riemannian Walk: si_step's gradient and path integral, a running Fisher
//                              F += alpha * (ge*ge - F) and, on a fold, the path score in F's metric    ia_adamw_step_segmented_rwalk
//       agem_step              consumed_step<agem_source>: g * s - alpha * r when g.r < 0     ia_adamw_step_segmented_projected
//       gem_step               consumed_step<gem_source>: g * s + sum_k v_k * r_k             ia_adamw_step_segmented_gem
//       masked_step            Piggyback, per tensor a kind: masked (the scores are trained on g * base and
//                              theta = score >= threshold ? base : 0), free (the plain rule), frozen    ia_adamw_step_segmented_masked
//       packed_step            PackNet, per tensor a kind: packed (the plain rule where owner == train_owner, nothing
//                              elsewhere), free, frozen                                          ia_adamw_step_segmented_packed
//       kinds_step             LoRA (csrc/lora.hip): free tensors take the plain rule, every other tensor is left alone; also
//                              the plain rule on the factor buffer with the caller's liveness flags   ia_adamw_step_segmented_kinds
//                              ia_adamw_step_segmented_grouped is the first four with lr and weight_decay per parameter group.
//   consumed_norm_kernel<Source>   the clip norm of the gradient a consumed_step consumes, from the SAME gradient functor
//                              (ia_grad_norm_projected, ia_grad_norm_gem, ia_grad_norm_packed); ia_grad_norm measures the raw gradient in the
//                              liveness pass.  grad_norm_finish_kernel adds the chunk sums of all three in a fixed order.
//   seg_step_advance_kernel    the per-tensor step counters and the clip / skip / projected / unsolved counters of every variant.
//   run_step                   liveness (activity pass or mark-all), the walker, the advance: three launches for every variant.
//   ia_pack_prune, ia_pack_apply   PackNet's pruning (an exact per-tensor radix select on |theta|) and owner map -> weights.
// The dots of A-GEM (ia_agem_dots) and GEM (ia_gem_dots, ia_gem_solve) run before their step and leave the decision on the device.
// OGD (ia_ogd_dots, ia_ogd_project) rewrites the flat gradient before a step it does not change.
// All are HBM-streaming kernels: 16-byte accesses, grid capped at 2048 workgroups, fp32 math.
#include "ia_common.h"
#include <type_traits>
#include <utility>

namespace {
constexpr int CL_THREADS = 256;
constexpr int CL_CHUNK = 4096;  // elements per chunk-table entry (host builds the table with this size)

__device__ __forceinline__ unsigned short bf16_bits(float x) {
    __hip_bfloat16 a = __float2bfloat16(x);
    return *reinterpret_cast<unsigned short*>(&a);
}

__device__ __forceinline__ ushort4 bf16_bits(float4 x) {
    ushort4 o;
    o.x = bf16_bits(x.x); o.y = bf16_bits(x.y); o.z = bf16_bits(x.z); o.w = bf16_bits(x.w);
    return o;
}

// W floats moved as one access: W = 4 in a chunk's float4 body (16 bytes), W = 1 in its tail
template <int W>
struct alignas(4 * W) vecf {
    float a[W];
    __device__ __forceinline__ float& operator[](int j) { return a[j]; }
    __device__ __forceinline__ float operator[](int j) const { return a[j]; }
};
template <int W> __device__ __forceinline__ vecf<W> ldv(const float* p, int64_t at) { return *reinterpret_cast<const vecf<W>*>(p + at); }
template <int W> __device__ __forceinline__ void stv(float* p, int64_t at, const vecf<W>& x) { *reinterpret_cast<vecf<W>*>(p + at) = x; }

__device__ __forceinline__ float block_sum(float v, float* sh) {
    v = ia_wave_sum_dpp(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < CL_THREADS / 64; ++i) t += sh[i];
    return t;
}

__global__ __launch_bounds__(CL_THREADS) void cl_penalty_kernel(
    const float* __restrict__ theta, const float* __restrict__ star, const float* __restrict__ w, float coef,
    float* __restrict__ grad, int accumulate, const int4* __restrict__ table, int nchunks,
    const float* __restrict__ seg_inv_numel, float* __restrict__ seg_abs_mean, float* __restrict__ penalty_sum) {
    __shared__ float sh[CL_THREADS / 64];
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int4 e = table[c];  // x = offset (multiple of 4), y = count, z = segment id
        const int off = e.x, cnt = e.y;
        float asum = 0.f, psum = 0.f;
        const int n4 = cnt >> 2;
        for (int q = threadIdx.x; q < n4; q += CL_THREADS) {
            const float4 t = reinterpret_cast<const float4*>(theta + off)[q];
            const float4 s = reinterpret_cast<const float4*>(star + off)[q];
            const float4 f = reinterpret_cast<const float4*>(w + off)[q];
            float4 d = make_float4(t.x - s.x, t.y - s.y, t.z - s.z, t.w - s.w);
            float4 g = make_float4(coef * f.x * d.x, coef * f.y * d.y, coef * f.z * d.z, coef * f.w * d.w);
            asum += fabsf(g.x) + fabsf(g.y) + fabsf(g.z) + fabsf(g.w);
            psum += f.x * d.x * d.x + f.y * d.y * d.y + f.z * d.z * d.z + f.w * d.w * d.w;
            if (grad) {
                float4* gp = reinterpret_cast<float4*>(grad + off) + q;
                if (accumulate) { const float4 o = *gp; g.x += o.x; g.y += o.y; g.z += o.z; g.w += o.w; }
                *gp = g;
            }
        }
        for (int i = (n4 << 2) + threadIdx.x; i < cnt; i += CL_THREADS) {
            const float d = theta[off + i] - star[off + i];
            float g = coef * w[off + i] * d;
            asum += fabsf(g);
            psum += w[off + i] * d * d;
            if (grad) grad[off + i] = accumulate ? grad[off + i] + g : g;
        }
        if (seg_abs_mean) {
            const float t = block_sum(asum, sh);
            if (threadIdx.x == 0) atomicAdd(seg_abs_mean + e.z, t * seg_inv_numel[e.z]);
        }
        if (penalty_sum) {
            const float t = block_sum(psum, sh);
            if (threadIdx.x == 0) atomicAdd(penalty_sum, t);
        }
    }
}

template <int MODE>  // 0: a += s*g*g (s read from device scalar)   1: a += |g|
__global__ __launch_bounds__(CL_THREADS) void cl_accumulate_kernel(float* __restrict__ acc, const float* __restrict__ g,
                                                                   const float* __restrict__ scalar, int64_t n) {
    const float s = (MODE == 0) ? scalar[0] : 1.f;
    const int64_t n4 = n >> 2;
    for (int64_t q = (int64_t)blockIdx.x * CL_THREADS + threadIdx.x; q < n4; q += (int64_t)gridDim.x * CL_THREADS) {
        float4 a = reinterpret_cast<float4*>(acc)[q];
        const float4 x = reinterpret_cast<const float4*>(g)[q];
        if (MODE == 0) { a.x += s * x.x * x.x; a.y += s * x.y * x.y; a.z += s * x.z * x.z; a.w += s * x.w * x.w; }
        else { a.x += fabsf(x.x); a.y += fabsf(x.y); a.z += fabsf(x.z); a.w += fabsf(x.w); }
        reinterpret_cast<float4*>(acc)[q] = a;
    }
    if (blockIdx.x == 0)
        for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += CL_THREADS)
            acc[i] += (MODE == 0) ? s * g[i] * g[i] : fabsf(g[i]);
}

// The unsegmented step (ia_adamw_step) only; the segmented steps use adamw1_rn
__device__ __forceinline__ void adamw1(float& p, float g, float& m, float& v, float lr, float b1, float b2, float eps,
                                       float wd, float step_size, float inv_bc2_sqrt) {
    p *= (1.f - lr * wd);
    m = m + (g - m) * (1.f - b1);                 // exp_avg.lerp_(grad, 1-beta1)
    v = v * b2 + (1.f - b2) * g * g;              // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1-beta2)
    const float denom = sqrtf(v) * inv_bc2_sqrt + eps;
    p -= step_size * (m / denom);
}

__global__ __launch_bounds__(CL_THREADS) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                           float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                           float lr, float b1, float b2, float eps, float wd,
                                                           float step_size, float inv_bc2_sqrt, float grad_scale,
                                                           unsigned short* __restrict__ shadow_bf16) {
    const int64_t n4 = n >> 2;
    for (int64_t q = (int64_t)blockIdx.x * CL_THREADS + threadIdx.x; q < n4; q += (int64_t)gridDim.x * CL_THREADS) {
        float4 P = reinterpret_cast<float4*>(p)[q];
        float4 G = reinterpret_cast<const float4*>(g)[q];
        float4 M = reinterpret_cast<float4*>(m)[q];
        float4 V = reinterpret_cast<float4*>(v)[q];
        adamw1(P.x, G.x * grad_scale, M.x, V.x, lr, b1, b2, eps, wd, step_size, inv_bc2_sqrt);
        adamw1(P.y, G.y * grad_scale, M.y, V.y, lr, b1, b2, eps, wd, step_size, inv_bc2_sqrt);
        adamw1(P.z, G.z * grad_scale, M.z, V.z, lr, b1, b2, eps, wd, step_size, inv_bc2_sqrt);
        adamw1(P.w, G.w * grad_scale, M.w, V.w, lr, b1, b2, eps, wd, step_size, inv_bc2_sqrt);
        reinterpret_cast<float4*>(p)[q] = P;
        reinterpret_cast<float4*>(m)[q] = M;
        reinterpret_cast<float4*>(v)[q] = V;
        if (shadow_bf16) reinterpret_cast<ushort4*>(shadow_bf16)[q] = bf16_bits(P);
    }
    if (blockIdx.x == 0)
        for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += CL_THREADS) {
            float P = p[i], M = m[i], V = v[i];
            adamw1(P, g[i] * grad_scale, M, V, lr, b1, b2, eps, wd, step_size, inv_bc2_sqrt);
            p[i] = P; m[i] = M; v[i] = V;
            if (shadow_bf16) shadow_bf16[i] = bf16_bits(P);
        }
}


// ---- per-tensor ("segment") AdamW: torch.optim.AdamW skips a parameter whose .grad is None (other languages' joint
// heads, heads of finished tasks) -- no weight decay, no moment decay, its own step counter.  With one flat gradient
// buffer "None" is "the segment received nothing since zero_grad": all-zero bits (or the host says every segment is
// live because a penalty was pre-loaded into .grad: R/utils.py:316-321 gives EVERY trainable tensor a gradient then).
// SUMSQ folds the first half of the gradient's L2 norm into the same pass over the raw gradient: workgroup c also leaves the
// fp32 sum of squares of chunk c in chunk_sumsq[c] with a plain store (no float atomics: grad_norm_finish_kernel adds the
// partials in a fixed order, so the norm reproduces bit for bit), and seg_active may then be NULL (every segment live: the
// caller memsets).  Rounding depth of one chunk sum: 4 (x*x + y*y + z*z + w*w) + 4 (a thread's <= 4 float4 of a
// 4096-element chunk) + 6 (DPP wave sum) + 3 (the four wave sums) = 17 fp32 roundings.
template <bool SUMSQ>
__global__ __launch_bounds__(CL_THREADS) void seg_activity_kernel(const float* __restrict__ g, const int4* __restrict__ table,
                                                                  int nchunks, int* __restrict__ seg_active,
                                                                  float* __restrict__ chunk_sumsq,
                                                                  const int* __restrict__ free_only_kind) {
    __shared__ float sh[CL_THREADS / 64];
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int4 e = table[c];
        if (!SUMSQ && free_only_kind && free_only_kind[e.z] != IA_MASK_FREE) continue;    // the step never looks at this flag
        const int off = e.x, cnt = e.y, n4 = cnt >> 2;
        unsigned nz = 0;
        float ss = 0.f;
        for (int q = threadIdx.x; q < n4; q += CL_THREADS) {
            const uint4 x = reinterpret_cast<const uint4*>(g + off)[q];
            nz |= (x.x | x.y | x.z | x.w) & 0x7FFFFFFFu;   // -0.0 counts as zero
            if constexpr (SUMSQ) {
                const float a = __uint_as_float(x.x), b = __uint_as_float(x.y), cc = __uint_as_float(x.z), d = __uint_as_float(x.w);
                ss += a * a + b * b + cc * cc + d * d;
            }
        }
        for (int i = (n4 << 2) + threadIdx.x; i < cnt; i += CL_THREADS) {
            nz |= __float_as_uint(g[off + i]) & 0x7FFFFFFFu;
            if constexpr (SUMSQ) ss += g[off + i] * g[off + i];
        }
        if ((!SUMSQ || seg_active) && __any(nz != 0) && (threadIdx.x & 63) == 0) atomicOr(seg_active + e.z, 1);
        if constexpr (SUMSQ) {
            const float t = block_sum(ss, sh);
            if (threadIdx.x == 0) chunk_sumsq[c] = t;
        }
    }
}

// Second half: ONE workgroup of GN_THREADS adds the chunk sums in fp64 in a fixed order -- wave w takes segments w, w + 16,
// ...; its lanes stride over the segment's chunks (contiguous in the table: seg_chunk_begin), then a butterfly over the
// lanes; the wave keeps a running fp64 total of its segments and thread 0 adds the 16 wave totals in order.
// norm_state = {total_norm, coef, non-finite flag (0 / 1), max_norm}.  `projected` (NULL, proj_state + 3 or gem_state +
// GEM_VIOLATED): a projected gradient already carries grad_scale, so the roots are scaled only when the step did not project.
constexpr int GN_THREADS = 1024;
__global__ __launch_bounds__(GN_THREADS) void grad_norm_finish_kernel(const float* __restrict__ chunk_sumsq,
                                                                      const int* __restrict__ seg_chunk_begin, int nseg,
                                                                      float abs_scale, float max_norm,
                                                                      float* __restrict__ seg_norm, float* __restrict__ norm_state,
                                                                      const float* __restrict__ projected) {
    __shared__ double sh_w[GN_THREADS / 64];
    if (projected && projected[0] != 0.f) abs_scale = 1.f;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double wave_total = 0.0;
    for (int s = wave; s < nseg; s += GN_THREADS / 64) {
        const int c0 = seg_chunk_begin[s], c1 = seg_chunk_begin[s + 1];
        double a = 0.0;
        for (int c = c0 + lane; c < c1; c += 64) a += (double)chunk_sumsq[c];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) a += __shfl_xor(a, d);
        if (lane == 0) seg_norm[s] = (float)sqrt(a) * abs_scale;
        wave_total += a;
    }
    if (lane == 0) sh_w[wave] = wave_total;
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = 0.0;
        for (int w = 0; w < GN_THREADS / 64; ++w) sum += sh_w[w];
        const float total = (float)sqrt(sum) * abs_scale;
        float coef = 1.f;
        if (max_norm > 0.f) {                      // clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max=1); NaN stays NaN
            coef = max_norm / (total + 1e-6f);
            if (coef > 1.f) coef = 1.f;
        }
        norm_state[0] = total;
        norm_state[1] = coef;
        norm_state[2] = isfinite(sum) ? 0.f : 1.f;
        norm_state[3] = max_norm;
    }
}

// Parameter groups: learning rate and weight decay per group, by value in the kernel arguments (the host fills them from two host
// arrays at every call: no copy, no staging buffer).  seg_group[k] is tensor k's group (NULL: group 0), so the lookup is
// workgroup-uniform per chunk: a scalar load of the index and two scalar loads from the argument segment.  It has to sit INSIDE
// the chunk loop: with more than 2048 chunks one workgroup visits chunks of different tensors.
struct group_table {
    int32_t n;
    float lr[IA_MAX_PARAM_GROUPS];
    float weight_decay[IA_MAX_PARAM_GROUPS];
};

__device__ __forceinline__ int group_of(const int* __restrict__ seg_group, int seg, int n) {
    const int gi = seg_group ? seg_group[seg] : 0;
    return gi < 0 ? 0 : (gi >= n ? n - 1 : gi);      // the argument segment is never indexed outside the table
}

// ---- the update rule of every segmented step.  Each product, difference and sum that forms the gradient AdamW consumes is
// rounded to fp32 on its own (contraction off), so that one torch op per rounding reproduces it bit for bit.
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

__device__ __forceinline__ float sub_rn(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}

__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

struct chunk_consts {   // workgroup-uniform operands of one chunk
    float decay, omb1, b2, omb2, eps, step_size, inv_bc2_sqrt, grad_scale, coef;
};

// CLIP: ge = g * grad_scale is multiplied by coef = norm_state[1], read from the device: two products, never fused with each
// other or into the moment update, so that with grad_scale == 1 the gradient is torch's g.mul_(coef) bit for bit.
template <bool CLIP>
__device__ __forceinline__ float eff_grad(float ge, const chunk_consts& k) {
    return CLIP ? mul_rn(ge, k.coef) : ge;
}

// torch.optim.AdamW's single-tensor update of one element, the definition for every segmented step:
//   v = b2 * v + (1 - b2) * g * g       as fma(g, (1-b2)*g, b2*v) in a chunk's float4 body and as fma(b2, v, ((1-b2)*g)*g) in its
//                                       scalar tail (TAIL): an element is in the body under every variant or in the tail under
//                                       every variant, so all of them move it alike
//   m = m + (1 - b1) * (g - m)          one fma on the separately rounded difference
//   p = decay * p - step_size * (m / (sqrt(v) * inv_bc2_sqrt + eps))     decay = 1 - lr * wd; denominator and result one fma each
// Nothing here is left to the compiler's contraction, which chose differently from kernel to kernel.
template <bool TAIL>
__device__ __forceinline__ void adamw1_rn(float& p, float g, float& m, float& v, float decay, const chunk_consts& k) {
#pragma clang fp contract(off)
    const float t = k.omb2 * g;
    if constexpr (TAIL) {
        const float tg = t * g;
        v = __builtin_fmaf(k.b2, v, tg);
    } else {
        const float vb = k.b2 * v;
        v = __builtin_fmaf(g, t, vb);
    }
    const float gm = g - m;
    m = __builtin_fmaf(k.omb1, gm, m);
    const float denom = __builtin_fmaf(k.inv_bc2_sqrt, sqrtf(v), k.eps);
    const float q = m / denom;
    const float u = k.step_size * q;
    p = __builtin_fmaf(decay, p, -u);
}

// A gradient functor maps W raw gradient elements at flat offset `at` to the gradient before the clip.  Its source is what the
// host passes; begin() reads the launch-uniform decision from the device once per workgroup.  The plain gradient: g * grad_scale.
struct scaled_grad {
    __device__ __forceinline__ scaled_grad begin() const { return *this; }
    __device__ __forceinline__ bool projecting() const { return false; }
    template <int W>
    __device__ __forceinline__ vecf<W> operator()(const vecf<W>& G, int64_t at, float grad_scale) const {
        vecf<W> a;
#pragma unroll
        for (int j = 0; j < W; ++j) a[j] = mul_rn(G[j], grad_scale);
        return a;
    }
};

// The rule of the steps that only change the gradient (plain, A-GEM, GEM): AdamW on grad(g) [* coef]
template <class Grad>
struct consumed_rule {
    Grad grad;
    static constexpr bool reads_theta = true;
    template <bool CLIP, int W>
    __device__ __forceinline__ void apply(vecf<W>& P, const vecf<W>& G, vecf<W>& M, vecf<W>& V, int64_t at,
                                          const chunk_consts& k) const {
        const vecf<W> E = grad(G, at, k.grad_scale);
#pragma unroll
        for (int j = 0; j < W; ++j) adamw1_rn<W == 1>(P[j], eff_grad<CLIP>(E[j], k), M[j], V[j], k.decay, k);
    }
};

template <class Source>
struct consumed_step {
    Source src;
    __device__ __forceinline__ auto begin() const { return consumed_rule<decltype(src.begin())>{src.begin()}; }
};
using plain_step = consumed_step<scaled_grad>;

// ---- Synaptic Intelligence (Zenke, Poole, Ganguli 2017) inside the AdamW launch.  Per element of a live tensor:
//   ge = g * grad_scale                      the task gradient (before the clip coefficient, without the penalty)
//   G  = ge [* coef] [+ (c2 * omega) * (theta - theta_star)]      the gradient AdamW consumes (PEN: a penalty is attached)
//   theta', m, v = adamw1_rn(theta, G, ...)
//   w  = w - ge * (theta' - theta)           the path integral, on the fp32 weight that is stored (weight decay included)
// A dead tensor's w stays.
template <bool PEN>
__device__ __forceinline__ float si_grad(float eff, float theta, float omega, float star, float c2) {
#pragma clang fp contract(off)
    if constexpr (!PEN) {
        return eff;
    } else {
        const float cw = c2 * omega;
        const float d = theta - star;
        const float pen = cw * d;
        return eff + pen;
    }
}

__device__ __forceinline__ float si_path(float w, float ge, float p_new, float p_old) {
#pragma clang fp contract(off)
    const float dp = p_new - p_old;
    const float t = ge * dp;
    return w - t;
}

template <bool PEN>
struct si_step {
    float* path_w; const float* omega; const float* star; float c2;
    static constexpr bool reads_theta = true;
    __device__ __forceinline__ si_step begin() const { return *this; }
    template <bool CLIP, int W>
    __device__ __forceinline__ void apply(vecf<W>& P, const vecf<W>& G, vecf<W>& M, vecf<W>& V, int64_t at,
                                          const chunk_consts& k) const {
        vecf<W> Pw = ldv<W>(path_w, at), O = {}, S = {};
        if constexpr (PEN) { O = ldv<W>(omega, at); S = ldv<W>(star, at); }
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const float ge = mul_rn(G[j], k.grad_scale), p_old = P[j];
            adamw1_rn<W == 1>(P[j], si_grad<PEN>(eff_grad<CLIP>(ge, k), p_old, O[j], S[j], c2), M[j], V[j], k.decay, k);
            Pw[j] = si_path(Pw[j], ge, P[j], p_old);
        }
        stv<W>(path_w, at, Pw);
    }
};

// End of a task: omega += max(0, w / ((theta - theta_star)^2 + xi)); w = 0; theta_star = theta.  One pass, 28 B per element.
__device__ __forceinline__ void si_consolidate1(float t, float& s, float& w, float& o, float xi) {
    const float d = t - s;
    o += fmaxf(0.f, w / (d * d + xi));
    w = 0.f;
    s = t;
}

__global__ __launch_bounds__(CL_THREADS) void si_consolidate_kernel(const float* __restrict__ theta, float* __restrict__ star,
                                                                    float* __restrict__ path_w, float* __restrict__ omega,
                                                                    float xi, int64_t n) {
    const int64_t n4 = n >> 2;
    for (int64_t q = (int64_t)blockIdx.x * CL_THREADS + threadIdx.x; q < n4; q += (int64_t)gridDim.x * CL_THREADS) {
        const float4 T = reinterpret_cast<const float4*>(theta)[q];
        float4 S = reinterpret_cast<float4*>(star)[q];
        float4 W = reinterpret_cast<float4*>(path_w)[q];
        float4 O = reinterpret_cast<float4*>(omega)[q];
        si_consolidate1(T.x, S.x, W.x, O.x, xi);
        si_consolidate1(T.y, S.y, W.y, O.y, xi);
        si_consolidate1(T.z, S.z, W.z, O.z, xi);
        si_consolidate1(T.w, S.w, W.w, O.w, xi);
        reinterpret_cast<float4*>(star)[q] = S;
        reinterpret_cast<float4*>(path_w)[q] = W;
        reinterpret_cast<float4*>(omega)[q] = O;
    }
    if (blockIdx.x == 0)
        for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += CL_THREADS) {
            float S = star[i], W = path_w[i], O = omega[i];
            si_consolidate1(theta[i], S, W, O, xi);
            star[i] = S; path_w[i] = W; omega[i] = O;
        }
}

// ---- Riemannian Walk (Chaudhry, Dokania, Ajanthan, Torr 2018) inside the AdamW launch: a running Fisher (EWC++) and, with
// SCORES, SI's path integral scored in that Fisher's metric.  Per element of a live tensor, each operation rounded on its own:
//   ge, G, theta', m, v       as si_step: the penalty (PEN) uses the consolidated importance, added after the clip
//   F' = F + alpha * (ge*ge - F)                       the moving average of the squared task gradient
//   w' = si_path(w, ge, theta', theta)                 (SCORES)
//   FOLD: score += max(0, w') / (0.5*F' * (theta' - anchor)^2 + eps);  w = 0;  anchor = theta'
// A variant loads and stores only what its flags need: 8 B per element for F, 8 for w, 16 for anchor and score, 8 for the penalty.
__device__ __forceinline__ float rw_fisher(float F, float ge, float alpha) {
#pragma clang fp contract(off)
    const float sq = ge * ge;
    const float df = sq - F;
    const float t = alpha * df;
    return F + t;
}

// One fold of the path integral into the score: six roundings on the increment (0.5 * F is exact)
__device__ __forceinline__ float rw_fold(float score, float w, float theta, float anchor, float F, float eps) {
#pragma clang fp contract(off)
    const float d = theta - anchor;
    const float dd = d * d;
    const float h = 0.5f * F;
    const float u = h * dd;
    const float den = u + eps;
    const float q = fmaxf(0.f, w) / den;
    return score + q;
}

template <bool PEN, bool SCORES, bool FOLD>
struct rwalk_step {
    static_assert(SCORES || !FOLD, "a fold needs the path integral");
    float *fisher, *path_w, *anchor, *score; const float *omega, *star; float c2, alpha, fold_eps;
    static constexpr bool reads_theta = true;
    __device__ __forceinline__ rwalk_step begin() const { return *this; }
    template <bool CLIP, int W>
    __device__ __forceinline__ void apply(vecf<W>& P, const vecf<W>& G, vecf<W>& M, vecf<W>& V, int64_t at,
                                          const chunk_consts& k) const {
        vecf<W> F = ldv<W>(fisher, at), Pw = {}, A = {}, Sc = {}, O = {}, S = {};
        if constexpr (SCORES) Pw = ldv<W>(path_w, at);
        if constexpr (FOLD) { A = ldv<W>(anchor, at); Sc = ldv<W>(score, at); }
        if constexpr (PEN) { O = ldv<W>(omega, at); S = ldv<W>(star, at); }
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const float ge = mul_rn(G[j], k.grad_scale), p_old = P[j];
            adamw1_rn<W == 1>(P[j], si_grad<PEN>(eff_grad<CLIP>(ge, k), p_old, O[j], S[j], c2), M[j], V[j], k.decay, k);
            F[j] = rw_fisher(F[j], ge, alpha);
            if constexpr (SCORES) Pw[j] = si_path(Pw[j], ge, P[j], p_old);
            if constexpr (FOLD) {
                Sc[j] = rw_fold(Sc[j], Pw[j], P[j], A[j], F[j], fold_eps);
                Pw[j] = 0.f;
            }
        }
        stv<W>(fisher, at, F);
        if constexpr (SCORES) stv<W>(path_w, at, Pw);
        if constexpr (FOLD) { stv<W>(anchor, at, P); stv<W>(score, at, Sc); }
    }
};

// End of a language, three launches, nothing read back and no float atomic (a maximum has no rounding: any order gives the bits).
//   rwalk_fold_max_kernel<SCORES>   workgroup c leaves {max F, max score} of chunk c in chunk_max[c]; with SCORES every element
//                                   is folded once more first (rw_fold; a dead tensor has w == 0: +0), w = 0, anchor = theta
//   rwalk_max_finish_kernel         one workgroup: maxima = {max F, max score} over all chunks
//   rwalk_combine_kernel<SCORES>    a = F / maxF, b = score / maxS (0 where the maximum is 0; F and score themselves when
//                                   !normalize); score_acc = first ? b : 0.5 * (score_acc + b); importance = a + score_acc
//                                   (a without SCORES); score = 0; theta_star = theta
// All buffers are >= 0 (F by its recurrence with alpha in (0, 1], score as a sum of max(0, .) quotients), so the maxima start at 0,
// which is also the value of the alignment gaps the chunk table does not visit.
__device__ __forceinline__ float block_max(float v, float* sh) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v = fmaxf(v, __shfl_xor(v, d));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    float t = sh[0];
#pragma unroll
    for (int i = 1; i < CL_THREADS / 64; ++i) t = fmaxf(t, sh[i]);
    return t;
}

template <bool SCORES, int W>
__device__ __forceinline__ void rwalk_fold_max_vec(const float* __restrict__ theta, const float* __restrict__ fisher,
                                                   float* __restrict__ path_w, float* __restrict__ anchor,
                                                   float* __restrict__ score, float eps, int at, float& mf, float& ms) {
    const vecf<W> F = ldv<W>(fisher, at);
#pragma unroll
    for (int j = 0; j < W; ++j) mf = fmaxf(mf, F[j]);
    if constexpr (SCORES) {
        const vecf<W> T = ldv<W>(theta, at), Pw = ldv<W>(path_w, at), A = ldv<W>(anchor, at);
        vecf<W> Sc = ldv<W>(score, at), Z = {};
#pragma unroll
        for (int j = 0; j < W; ++j) {
            Sc[j] = rw_fold(Sc[j], Pw[j], T[j], A[j], F[j], eps);
            ms = fmaxf(ms, Sc[j]);
        }
        stv<W>(score, at, Sc);
        stv<W>(path_w, at, Z);
        stv<W>(anchor, at, T);
    }
}

template <bool SCORES>
__global__ __launch_bounds__(CL_THREADS) void rwalk_fold_max_kernel(const float* __restrict__ theta,
                                                                    const float* __restrict__ fisher, float* __restrict__ path_w,
                                                                    float* __restrict__ anchor, float* __restrict__ score,
                                                                    float eps, const int4* __restrict__ table, int nchunks,
                                                                    float2* __restrict__ chunk_max) {
    __shared__ float sh[CL_THREADS / 64];
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int4 e = table[c];
        const int off = e.x, cnt = e.y, n4 = cnt >> 2;
        float mf = 0.f, ms = 0.f;
        for (int q = threadIdx.x; q < n4; q += CL_THREADS)
            rwalk_fold_max_vec<SCORES, 4>(theta, fisher, path_w, anchor, score, eps, off + (q << 2), mf, ms);
        for (int i = (n4 << 2) + threadIdx.x; i < cnt; i += CL_THREADS)
            rwalk_fold_max_vec<SCORES, 1>(theta, fisher, path_w, anchor, score, eps, off + i, mf, ms);
        mf = block_max(mf, sh);
        if constexpr (SCORES) ms = block_max(ms, sh);
        if (threadIdx.x == 0) chunk_max[c] = make_float2(mf, ms);
    }
}

__global__ __launch_bounds__(CL_THREADS) void rwalk_max_finish_kernel(const float2* __restrict__ chunk_max, int nchunks,
                                                                      float* __restrict__ maxima) {
    __shared__ float sh[CL_THREADS / 64];
    float mf = 0.f, ms = 0.f;
    for (int c = threadIdx.x; c < nchunks; c += CL_THREADS) {
        const float2 x = chunk_max[c];
        mf = fmaxf(mf, x.x);
        ms = fmaxf(ms, x.y);
    }
    mf = block_max(mf, sh);
    ms = block_max(ms, sh);
    if (threadIdx.x == 0) { maxima[0] = mf; maxima[1] = ms; }
}

__device__ __forceinline__ float rw_share(float x, float mx, bool normalize) {
    return !normalize ? x : (mx == 0.f ? 0.f : x / mx);
}

template <bool SCORES, int W>
__device__ __forceinline__ void rwalk_combine_vec(const float* __restrict__ theta, float* __restrict__ star,
                                                  const float* __restrict__ fisher, float* __restrict__ score,
                                                  float* __restrict__ score_acc, float* __restrict__ importance, float mf,
                                                  float ms, bool normalize, bool first, int64_t at) {
    const vecf<W> F = ldv<W>(fisher, at);
    vecf<W> Om;
    if constexpr (SCORES) {
        const vecf<W> Sc = ldv<W>(score, at);
        vecf<W> Acc = {}, Z = {};
        if (!first) Acc = ldv<W>(score_acc, at);
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const float b = rw_share(Sc[j], ms, normalize);
            Acc[j] = first ? b : mul_rn(0.5f, add_rn(Acc[j], b));
            Om[j] = add_rn(rw_share(F[j], mf, normalize), Acc[j]);
        }
        stv<W>(score_acc, at, Acc);
        stv<W>(score, at, Z);
    } else {
#pragma unroll
        for (int j = 0; j < W; ++j) Om[j] = rw_share(F[j], mf, normalize);
    }
    stv<W>(importance, at, Om);
    stv<W>(star, at, ldv<W>(theta, at));
}

template <bool SCORES>
__global__ __launch_bounds__(CL_THREADS) void rwalk_combine_kernel(const float* __restrict__ theta, float* __restrict__ star,
                                                                   const float* __restrict__ fisher, float* __restrict__ score,
                                                                   float* __restrict__ score_acc, float* __restrict__ importance,
                                                                   const float* __restrict__ maxima, int normalize, int first,
                                                                   int64_t n) {
    const float mf = maxima[0], ms = maxima[1];
    const int64_t n4 = n >> 2;
    for (int64_t q = (int64_t)blockIdx.x * CL_THREADS + threadIdx.x; q < n4; q += (int64_t)gridDim.x * CL_THREADS)
        rwalk_combine_vec<SCORES, 4>(theta, star, fisher, score, score_acc, importance, mf, ms, normalize, first, q << 2);
    if (blockIdx.x == 0)
        for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += CL_THREADS)
            rwalk_combine_vec<SCORES, 1>(theta, star, fisher, score, score_acc, importance, mf, ms, normalize, first, i);
}

// ---- Averaged GEM (Chaudhry, Ranzato, Rohrbach, Elhoseiny 2019).  r is the gradient of a batch drawn from the episodic memory,
// stored averaged and in true units; g is the flat task gradient, still to be multiplied by grad_scale.  When g.r < 0 the step
// consumes g - (g.r / r.r) * r.  Three passes, none with a float atomic, each with a fixed summation order:
//   agem_dots_kernel     workgroup c leaves {sum g*r, sum r*r} of chunk c (fp32, the reduction shape of
//                        seg_activity_kernel<true>) in chunk_dots[c] and sets the liveness flags from g as that kernel does
//   agem_finish_kernel   one workgroup adds the partials in fp64 (thread t takes chunks t, t + 1024, ...; butterfly over the
//                        lanes; thread 0 adds the 16 wave totals in order) and writes proj_state = {dot, ref_sq, alpha, violated}
//   consumed_norm_kernel<agem_source>   the chunk sums of squares of the gradient the step will consume, branching on the
//                        device flag
__global__ __launch_bounds__(CL_THREADS) void agem_dots_kernel(const float* __restrict__ g, const float* __restrict__ r,
                                                               const int4* __restrict__ table, int nchunks,
                                                               int* __restrict__ seg_active, float2* __restrict__ chunk_dots) {
    __shared__ float sh[CL_THREADS / 64];
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int4 e = table[c];
        const int off = e.x, cnt = e.y, n4 = cnt >> 2;
        unsigned nz = 0;
        float gr = 0.f, rr = 0.f;
        for (int q = threadIdx.x; q < n4; q += CL_THREADS) {
            const uint4 x = reinterpret_cast<const uint4*>(g + off)[q];
            const float4 y = reinterpret_cast<const float4*>(r + off)[q];
            nz |= (x.x | x.y | x.z | x.w) & 0x7FFFFFFFu;   // -0.0 counts as zero
            const float a = __uint_as_float(x.x), b = __uint_as_float(x.y), cc = __uint_as_float(x.z), d = __uint_as_float(x.w);
            gr += a * y.x + b * y.y + cc * y.z + d * y.w;
            rr += y.x * y.x + y.y * y.y + y.z * y.z + y.w * y.w;
        }
        for (int i = (n4 << 2) + threadIdx.x; i < cnt; i += CL_THREADS) {
            const float a = g[off + i], y = r[off + i];
            nz |= __float_as_uint(a) & 0x7FFFFFFFu;
            gr += a * y;
            rr += y * y;
        }
        if (seg_active && __any(nz != 0) && (threadIdx.x & 63) == 0) atomicOr(seg_active + e.z, 1);
        const float t0 = block_sum(gr, sh);
        const float t1 = block_sum(rr, sh);
        if (threadIdx.x == 0) chunk_dots[c] = make_float2(t0, t1);
    }
}

__global__ __launch_bounds__(GN_THREADS) void agem_finish_kernel(const float2* __restrict__ chunk_dots, int nchunks,
                                                                 float grad_scale, float* __restrict__ proj_state) {
    __shared__ double sh_d[GN_THREADS / 64], sh_r[GN_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double d = 0.0, q = 0.0;
    for (int c = threadIdx.x; c < nchunks; c += GN_THREADS) {
        const float2 p = chunk_dots[c];
        d += (double)p.x;
        q += (double)p.y;
    }
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) { d += __shfl_xor(d, s); q += __shfl_xor(q, s); }
    if (lane == 0) { sh_d[wave] = d; sh_r[wave] = q; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sd = 0.0, sq = 0.0;
        for (int w = 0; w < GN_THREADS / 64; ++w) { sd += sh_d[w]; sq += sh_r[w]; }
        const double dot = (double)grad_scale * sd;
        const bool violated = isfinite(dot) && isfinite(sq) && dot < 0.0 && sq > 0.0;   // a non-finite g or r never projects
        proj_state[0] = (float)dot;
        proj_state[1] = (float)sq;
        proj_state[2] = violated ? (float)(dot / sq) : 0.f;    // the quotient in fp64, rounded once
        proj_state[3] = violated ? 1.f : 0.f;
    }
}

// (g * grad_scale) - (alpha * r) when the step projects: both products and the difference rounded to fp32 on their own.  An
// un-projected step does not read r.  Liveness is that of the task gradient g, whatever r holds.
struct agem_grad {
    const float* ref; float alpha; bool violated;      // violated: uniform over the launch
    __device__ __forceinline__ bool projecting() const { return violated; }
    template <int W>
    __device__ __forceinline__ vecf<W> operator()(const vecf<W>& G, int64_t at, float grad_scale) const {
        vecf<W> a, R = {};
        if (violated) R = ldv<W>(ref, at);
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const float ge = mul_rn(G[j], grad_scale);
            a[j] = violated ? sub_rn(ge, mul_rn(alpha, R[j])) : ge;
        }
        return a;
    }
};

struct agem_source {
    const float* ref; const float* proj_state;
    __device__ __forceinline__ agem_grad begin() const { return {ref, proj_state[2], proj_state[3] != 0.f}; }
};
using agem_step = consumed_step<agem_source>;


// ---- GEM (Lopez-Paz, Ranzato 2017): one constraint per earlier task.  refs is [max_tasks, stride] fp32, row k the reference
// gradient of task k laid out as grad; K = ntasks rows are in use.  gem_sums (IA_GEM_SUMS_DOUBLES doubles) = d[16], then the
// Gram matrix [16, 16]: the fp64 sums as the finish kernel left them, which is what the solver consumes.  gem_state
// (IA_GEM_STATE_FLOATS floats) = v[16], violated, active, iterations, solved.
//   gem_dots_kernel      workgroup c holds chunk c of x in registers (a 4096-element chunk is four float4 per thread), reads each
//                        of the K rows once and leaves the K fp32 sums in chunk_dots[c * K + k]; per row the thread's partial,
//                        the DPP wave sum and the four wave sums in order: the reduction shape of agem_dots_kernel
//   gem_finish_kernel    one workgroup adds the partials in fp64 (agem_finish_kernel's order) and writes d, or row and column
//                        gram_row of the Gram matrix
//   gem_solve_kernel     the bound-constrained QP in fp64, by an active-set method
//   consumed_norm_kernel<gem_source>, adamw_seg_kernel<CLIP, gem_step>   norm and step on g * s + sum_k v_k * r_k
constexpr int GEM_MAX = IA_GEM_MAX_TASKS;
constexpr int GEM_V = 0, GEM_VIOLATED = GEM_MAX, GEM_ACTIVE = GEM_VIOLATED + 1, GEM_ITERATIONS = GEM_VIOLATED + 2,
              GEM_SOLVED = GEM_VIOLATED + 3;
constexpr int GEM_D = 0, GEM_GRAM = GEM_MAX;                  // offsets into gem_sums
constexpr int GEM_CHUNK_F4 = CL_CHUNK / (4 * CL_THREADS);   // float4 of a full chunk per thread
static_assert(GEM_CHUNK_F4 * 4 * CL_THREADS == CL_CHUNK && IA_GEM_STATE_FLOATS == GEM_SOLVED + 1 &&
              IA_GEM_SUMS_DOUBLES == GEM_GRAM + GEM_MAX * GEM_MAX, "GEM layout");

__global__ __launch_bounds__(CL_THREADS) void gem_dots_kernel(const float* __restrict__ x, const float* __restrict__ refs,
                                                              int64_t stride, int K, const int4* __restrict__ table, int nchunks,
                                                              int* __restrict__ seg_active, float* __restrict__ chunk_dots) {
    __shared__ float sh[GEM_MAX][CL_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int4 e = table[c];
        const int off = e.x, cnt = e.y, n4 = cnt >> 2;    // cnt <= CL_CHUNK: at most GEM_CHUNK_F4 float4 per thread
        const int tail = (n4 << 2) + threadIdx.x;          // the chunk's last cnt & 3 elements, one per thread
        float4 X[GEM_CHUNK_F4];
        unsigned nz = 0;
#pragma unroll
        for (int u = 0; u < GEM_CHUNK_F4; ++u) {
            const int q = threadIdx.x + u * CL_THREADS;
            X[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (q < n4) X[u] = reinterpret_cast<const float4*>(x + off)[q];
            nz |= (__float_as_uint(X[u].x) | __float_as_uint(X[u].y) | __float_as_uint(X[u].z) | __float_as_uint(X[u].w)) &
                  0x7FFFFFFFu;                             // -0.0 counts as zero
        }
        const float xt = tail < cnt ? x[off + tail] : 0.f;
        nz |= __float_as_uint(xt) & 0x7FFFFFFFu;
        if (seg_active && __any(nz != 0) && lane == 0) atomicOr(seg_active + e.z, 1);
        for (int k = 0; k < K; ++k) {
            const float* __restrict__ r = refs + (int64_t)k * stride + off;
            float a = 0.f;
#pragma unroll
            for (int u = 0; u < GEM_CHUNK_F4; ++u) {
                const int q = threadIdx.x + u * CL_THREADS;
                if (q < n4) {
                    const float4 y = reinterpret_cast<const float4*>(r)[q];
                    a += X[u].x * y.x + X[u].y * y.y + X[u].z * y.z + X[u].w * y.w;
                }
            }
            if (tail < cnt) a += xt * r[tail];
            a = ia_wave_sum_dpp(a);
            if (lane == 0) sh[k][wave] = a;
        }
        __syncthreads();
        if (threadIdx.x < K) {
            float t = 0.f;
#pragma unroll
            for (int i = 0; i < CL_THREADS / 64; ++i) t += sh[threadIdx.x][i];
            chunk_dots[(int64_t)c * K + threadIdx.x] = t;
        }
        __syncthreads();
    }
}

// gram_row < 0: d[k] = scale * sum (k < K), 0 beyond.  Otherwise gram[gram_row][k] = gram[k][gram_row] = sum (k < K).
__global__ __launch_bounds__(GN_THREADS) void gem_finish_kernel(const float* __restrict__ chunk_dots, int nchunks, int K,
                                                                float scale, int gram_row, double* __restrict__ gem_sums) {
    __shared__ double sh_d[GN_THREADS / 64][GEM_MAX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double a[GEM_MAX];
#pragma unroll
    for (int k = 0; k < GEM_MAX; ++k) a[k] = 0.0;
    for (int c = threadIdx.x; c < nchunks; c += GN_THREADS) {
        const float* p = chunk_dots + (int64_t)c * K;
#pragma unroll
        for (int k = 0; k < GEM_MAX; ++k)
            if (k < K) a[k] += (double)p[k];
    }
#pragma unroll
    for (int k = 0; k < GEM_MAX; ++k) {
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) a[k] += __shfl_xor(a[k], s);
        if (lane == 0) sh_d[wave][k] = a[k];
    }
    __syncthreads();
    if (threadIdx.x < GEM_MAX) {
        const int k = threadIdx.x;
        double sum = 0.0;
        for (int w = 0; w < GN_THREADS / 64; ++w) sum += sh_d[w][k];
        if (gram_row < 0) {
            gem_sums[GEM_D + k] = k < K ? (double)scale * sum : 0.0;
        } else if (k < K) {
            gem_sums[GEM_GRAM + gram_row * GEM_MAX + k] = sum;
            gem_sums[GEM_GRAM + k * GEM_MAX + gram_row] = sum;
        }
    }
}

// v = argmin 1/2 v'Pv + d'v subject to v >= gamma, P = gram + eps I (K x K), in fp64 by the active-set method of Lawson and
// Hanson's NNLS carried over to a lower bound: F is the set of free coordinates, every other one sits at gamma.  Outer step: the
// bound coordinate with the most negative multiplier lambda_j = (Pv + d)_j joins F; inner steps: the minimiser z of the face
// (Cholesky of P_FF) is taken whole when it is inside the bounds, otherwise v moves towards z up to the first bound and the
// coordinates that reached it leave F.  Every completed outer step lowers the objective on a face not visited before, so the
// method ends after finitely many; K <= 16 needs a handful, and GEM_SOLVE_CAP is there for inputs no arithmetic can serve.
// One lane does the work: the systems are at most 16 x 16 and every step depends on the one before.
constexpr int GEM_SOLVE_CAP = 256;

__device__ bool gem_face_minimiser(const double (*P)[GEM_MAX], double (*L)[GEM_MAX], const double* d, int K, unsigned free_set,
                                   double gamma, double* z) {
    int idx[GEM_MAX], n = 0;
    for (int k = 0; k < K; ++k)
        if (free_set >> k & 1u) idx[n++] = k;
    double b[GEM_MAX];
    for (int i = 0; i < n; ++i) {
        double rhs = -d[idx[i]];
        for (int k = 0; k < K; ++k)
            if (!(free_set >> k & 1u)) rhs -= P[idx[i]][k] * gamma;
        b[i] = rhs;
    }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = P[idx[i]][idx[j]];
            for (int t = 0; t < j; ++t) s -= L[i][t] * L[j][t];
            if (i == j) {
                if (!(s > 0.0)) return false;       // not positive definite (or NaN)
                L[i][i] = sqrt(s);
            } else {
                L[i][j] = s / L[j][j];
            }
        }
    for (int i = 0; i < n; ++i) {
        double s = b[i];
        for (int t = 0; t < i; ++t) s -= L[i][t] * b[t];
        b[i] = s / L[i][i];
    }
    for (int i = n - 1; i >= 0; --i) {
        double s = b[i];
        for (int t = i + 1; t < n; ++t) s -= L[t][i] * b[t];
        b[i] = s / L[i][i];
    }
    for (int k = 0; k < K; ++k) z[k] = gamma;
    for (int i = 0; i < n; ++i) z[idx[i]] = b[i];
    return true;
}

__global__ __launch_bounds__(64) void gem_solve_kernel(const double* __restrict__ gem_sums, float* __restrict__ gem_state, int K,
                                                       float gamma_f, float eps_f) {
    __shared__ double P[GEM_MAX][GEM_MAX], L[GEM_MAX][GEM_MAX], d[GEM_MAX], v[GEM_MAX], z[GEM_MAX];
    if (threadIdx.x != 0) return;
    const double gamma = (double)gamma_f;
    bool finite = true, violated = false;
    double scale = 0.0;
    for (int k = 0; k < K; ++k) {
        d[k] = gem_sums[GEM_D + k];
        finite = finite && isfinite(d[k]);
        violated = violated || d[k] < 0.0;
        scale = fmax(scale, fabs(d[k]));
        double row = 0.0;
        for (int j = 0; j < K; ++j) {
            P[k][j] = gem_sums[GEM_GRAM + k * GEM_MAX + j] + (j == k ? (double)eps_f : 0.0);
            finite = finite && isfinite(P[k][j]);
            row += fabs(P[k][j]);
        }
        scale = fmax(scale, row * fmax(gamma, 1.0));
    }
    int iterations = 0, active = 0;
    bool solved = finite;
    violated = violated && finite;
    for (int k = 0; k < GEM_MAX; ++k) v[k] = 0.0;
    if (violated) {
        const double tol = 1e-12 * scale;          // on a multiplier: what its own fp64 evaluation cannot resolve
        unsigned free_set = 0, refused = 0;        // refused: the face's minimiser did not take it inside; not offered again here
        for (int k = 0; k < K; ++k) v[k] = gamma;
        solved = false;
        bool ok = true;
        while (ok && iterations < GEM_SOLVE_CAP) {
            int j = -1;
            double worst = -tol;
            for (int k = 0; k < K; ++k) {
                if ((free_set | refused) >> k & 1u) continue;
                double lam = d[k];
                for (int t = 0; t < K; ++t) lam += P[k][t] * v[t];
                if (lam < worst) { worst = lam; j = k; }
            }
            if (j < 0) { solved = true; break; }
            free_set |= 1u << j;
            bool first = true;
            while (free_set && iterations < GEM_SOLVE_CAP) {
                ++iterations;
                ok = gem_face_minimiser(P, L, d, K, free_set, gamma, z);
                if (!ok) break;
                if (first && !(z[j] > gamma)) {     // in exact arithmetic a negative multiplier always moves inside
                    free_set &= ~(1u << j);
                    refused |= 1u << j;
                    break;
                }
                if (first) refused = 0;
                first = false;
                int kb = -1;
                double alpha = 1.0;
                for (int k = 0; k < K; ++k)
                    if ((free_set >> k & 1u) && !(z[k] > gamma)) {
                        const double room = v[k] - gamma, a = room <= 0.0 ? 0.0 : room / (v[k] - z[k]);
                        if (a <= alpha) { alpha = a; kb = k; }
                    }
                if (kb < 0) {                       // the minimiser of the face lies inside the bounds: take it whole
                    for (int k = 0; k < K; ++k) v[k] = z[k];
                    break;
                }
                for (int k = 0; k < K; ++k)
                    if (free_set >> k & 1u) {
                        v[k] += alpha * (z[k] - v[k]);
                        if (k == kb || !(v[k] > gamma)) { v[k] = gamma; free_set &= ~(1u << k); }
                    }
            }
        }
        for (int k = 0; k < K; ++k) solved = solved && isfinite((double)(float)v[k]);
        if (!solved) {
            violated = false;
            for (int k = 0; k < K; ++k) v[k] = 0.0;
        }
        for (int k = 0; k < K; ++k) active += v[k] > gamma ? 1 : 0;
    }
    for (int k = 0; k < GEM_MAX; ++k) gem_state[GEM_V + k] = (float)v[k];
    gem_state[GEM_VIOLATED] = violated ? 1.f : 0.f;
    gem_state[GEM_ACTIVE] = (float)active;
    gem_state[GEM_ITERATIONS] = (float)iterations;
    gem_state[GEM_SOLVED] = solved ? 1.f : 0.f;
}

// acc = g * s, then acc += v_k * r_k for k ascending over the rows with v_k != 0: every product and sum rounded on its own.
// K = 0 when the step does not project: no row is read.
struct gem_grad {
    const float* refs; int64_t stride; int K; const float* sh_v;     // K: uniform over the launch
    __device__ __forceinline__ bool projecting() const { return K > 0; }
    template <int W>
    __device__ __forceinline__ vecf<W> operator()(const vecf<W>& G, int64_t at, float grad_scale) const {
        vecf<W> a;
#pragma unroll
        for (int j = 0; j < W; ++j) a[j] = mul_rn(G[j], grad_scale);
        for (int k = 0; k < K; ++k) {
            const float vk = sh_v[k];
            if (vk == 0.f) continue;                 // workgroup-uniform: the row is not read
            const vecf<W> R = ldv<W>(refs + (int64_t)k * stride, at);
#pragma unroll
            for (int j = 0; j < W; ++j) a[j] = add_rn(a[j], mul_rn(vk, R[j]));
        }
        return a;
    }
};

struct gem_source {
    const float* refs; int64_t stride; int ntasks; const float* gem_state;
    __device__ __forceinline__ gem_grad begin() const {
        __shared__ float sh_v[GEM_MAX];
        if (threadIdx.x < GEM_MAX) sh_v[threadIdx.x] = gem_state[GEM_V + threadIdx.x];
        __syncthreads();
        return {refs, stride, gem_state[GEM_VIOLATED] != 0.f ? ntasks : 0, sh_v};
    }
};
using gem_step = consumed_step<gem_source>;

// ---- Orthogonal Gradient Descent (Farajtabar, Azizan, Mott, Li 2020): basis is [max_rows, stride] fp32, rows 0 .. nrows-1
// orthonormal and laid out as grad, zero outside the scope (seg_scope[k] != 0: tensor k is projected).  Every step consumes
// x - sum_k <x, v_k> v_k.  No sign test and no program: the dots, then the projection, both pure streaming.
//   ogd_dots_kernel      workgroup c holds chunk c of x in registers (gem_dots_kernel's layout), streams the rows in tiles of
//                        OGD_TILE and leaves the fp32 sums in partials[k * nchunks + c]: one line of the workspace per row, so
//                        that the finisher reads each row's partials contiguously.  Per row the thread's partial, the DPP wave
//                        sum and the four wave sums in order: the reduction shape of agem_dots_kernel.  SQ: line nrows holds
//                        sum x*x of the chunk (the shape of seg_activity_kernel<true>).  A chunk outside the scope stores zeros
//                        and reads x only for the liveness flags.
//   ogd_finish_kernel    workgroup k adds line k in fp64 (agem_finish_kernel's order) and writes the sum as fp64 and, rounded
//                        once, as fp32: one workgroup per row, so 4096 rows cost what 16 do per row.
//   ogd_project_kernel   acc = x; for k ascending: acc = acc - c_k * v_k; dst = acc * alpha, every product and difference
//                        rounded on its own.  x and dst may be the same buffer, so neither is __restrict__.
constexpr int OGD_TILE = 16;   // rows between two barriers of the dots kernel
constexpr int OGD_ROWS = 4;    // rows whose loads are issued together (dots and projection): 16 float4 in flight per thread

struct ogd_chunk {             // chunk c of x as the thread holds it
    float4 X[GEM_CHUNK_F4];
    float xt;                  // one of the chunk's last cnt & 3 elements, or 0
};

__device__ __forceinline__ ogd_chunk ogd_load_chunk(const float* x, int off, int cnt) {
    const int n4 = cnt >> 2, tail = (n4 << 2) + threadIdx.x;
    ogd_chunk h;
#pragma unroll
    for (int u = 0; u < GEM_CHUNK_F4; ++u) {
        const int q = threadIdx.x + u * CL_THREADS;
        h.X[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q < n4) h.X[u] = reinterpret_cast<const float4*>(x + off)[q];
    }
    h.xt = tail < cnt ? x[off + tail] : 0.f;
    return h;
}

// the thread's share of <x, r> over one chunk; r points at the chunk's first element of the row
__device__ __forceinline__ float ogd_row_partial(const ogd_chunk& h, const float* __restrict__ r, int cnt) {
    const int n4 = cnt >> 2, tail = (n4 << 2) + threadIdx.x;
    float4 y[GEM_CHUNK_F4];
#pragma unroll
    for (int u = 0; u < GEM_CHUNK_F4; ++u) {
        const int q = threadIdx.x + u * CL_THREADS;
        y[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q < n4) y[u] = reinterpret_cast<const float4*>(r)[q];
    }
    float a = 0.f;
#pragma unroll
    for (int u = 0; u < GEM_CHUNK_F4; ++u)
        if (threadIdx.x + u * CL_THREADS < n4) a += h.X[u].x * y[u].x + h.X[u].y * y[u].y + h.X[u].z * y[u].z + h.X[u].w * y[u].w;
    if (tail < cnt) a += h.xt * r[tail];
    return a;
}

template <bool SQ>
__global__ __launch_bounds__(CL_THREADS) void ogd_dots_kernel(const float* __restrict__ x, const float* __restrict__ basis,
                                                              int64_t stride, int nrows, const int4* __restrict__ table,
                                                              int nchunks, const int* __restrict__ seg_scope,
                                                              int* __restrict__ seg_active, float* __restrict__ partials) {
    __shared__ float sh[OGD_TILE][CL_THREADS / 64];
    __shared__ float sh_sq[CL_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lines = nrows + (SQ ? 1 : 0);
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int4 e = table[c];
        const int off = e.x, cnt = e.y;                    // cnt <= CL_CHUNK: at most GEM_CHUNK_F4 float4 per thread
        const bool in_scope = seg_scope[e.z] != 0;
        if (!in_scope && !seg_active) {
            for (int k = threadIdx.x; k < lines; k += CL_THREADS) partials[(int64_t)k * nchunks + c] = 0.f;
            continue;
        }
        const ogd_chunk h = ogd_load_chunk(x, off, cnt);
        if (seg_active) {
            unsigned nz = __float_as_uint(h.xt);
#pragma unroll
            for (int u = 0; u < GEM_CHUNK_F4; ++u)
                nz |= __float_as_uint(h.X[u].x) | __float_as_uint(h.X[u].y) | __float_as_uint(h.X[u].z) | __float_as_uint(h.X[u].w);
            if (__any((nz & 0x7FFFFFFFu) != 0) && lane == 0) atomicOr(seg_active + e.z, 1);    // -0.0 counts as zero
        }
        if (!in_scope) {
            for (int k = threadIdx.x; k < lines; k += CL_THREADS) partials[(int64_t)k * nchunks + c] = 0.f;
            continue;
        }
        if constexpr (SQ) {
            float ss = 0.f;
#pragma unroll
            for (int u = 0; u < GEM_CHUNK_F4; ++u)
                ss += h.X[u].x * h.X[u].x + h.X[u].y * h.X[u].y + h.X[u].z * h.X[u].z + h.X[u].w * h.X[u].w;
            ss += h.xt * h.xt;
            const float t = block_sum(ss, sh_sq);
            if (threadIdx.x == 0) partials[(int64_t)nrows * nchunks + c] = t;
        }
        for (int k0 = 0; k0 < nrows; k0 += OGD_TILE) {
            const int kt = nrows - k0 < OGD_TILE ? nrows - k0 : OGD_TILE;
            const float* r0 = basis + (int64_t)k0 * stride + off;
            int k = 0;
            for (; k + OGD_ROWS <= kt; k += OGD_ROWS) {
                float a[OGD_ROWS];
#pragma unroll
                for (int j = 0; j < OGD_ROWS; ++j) a[j] = ogd_row_partial(h, r0 + (int64_t)(k + j) * stride, cnt);
#pragma unroll
                for (int j = 0; j < OGD_ROWS; ++j) {
                    a[j] = ia_wave_sum_dpp(a[j]);
                    if (lane == 0) sh[k + j][wave] = a[j];
                }
            }
            for (; k < kt; ++k) {
                const float a = ia_wave_sum_dpp(ogd_row_partial(h, r0 + (int64_t)k * stride, cnt));
                if (lane == 0) sh[k][wave] = a;
            }
            __syncthreads();
            if (threadIdx.x < kt) {
                float t = 0.f;
#pragma unroll
                for (int i = 0; i < CL_THREADS / 64; ++i) t += sh[threadIdx.x][i];
                partials[(int64_t)(k0 + threadIdx.x) * nchunks + c] = t;
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(GN_THREADS) void ogd_finish_kernel(const float* __restrict__ partials, int nchunks,
                                                                double* __restrict__ dots64, float* __restrict__ dots32) {
    __shared__ double sh_d[GN_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* line = partials + (int64_t)blockIdx.x * nchunks;
    double d = 0.0;
    for (int c = threadIdx.x; c < nchunks; c += GN_THREADS) d += (double)line[c];
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) d += __shfl_xor(d, s);
    if (lane == 0) sh_d[wave] = d;
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = 0.0;
        for (int w = 0; w < GN_THREADS / 64; ++w) sum += sh_d[w];
        dots64[blockIdx.x] = sum;
        dots32[blockIdx.x] = (float)sum;
    }
}

__global__ __launch_bounds__(CL_THREADS) void ogd_project_kernel(const float* x, const float* __restrict__ basis, int64_t stride,
                                                                 int nrows, const float* __restrict__ coef, float alpha,
                                                                 const int4* __restrict__ table, int nchunks,
                                                                 const int* __restrict__ seg_scope,
                                                                 const int* __restrict__ seg_active, float* dst) {
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int4 e = table[c];
        const int off = e.x, cnt = e.y, n4 = cnt >> 2, tail = (n4 << 2) + threadIdx.x;
        if (seg_scope[e.z] == 0) {
            if (dst != x) {                                // a basis row is zero outside the scope
#pragma unroll
                for (int u = 0; u < GEM_CHUNK_F4; ++u) {
                    const int q = threadIdx.x + u * CL_THREADS;
                    if (q < n4) reinterpret_cast<float4*>(dst + off)[q] = make_float4(0.f, 0.f, 0.f, 0.f);
                }
                if (tail < cnt) dst[off + tail] = 0.f;
            }
            continue;
        }
        if (seg_active && seg_active[e.z] == 0) continue;
        ogd_chunk h = ogd_load_chunk(x, off, cnt);
        const float* r0 = basis + off;
        int k = 0;
        for (; k + OGD_ROWS <= nrows; k += OGD_ROWS) {
            float4 y[OGD_ROWS][GEM_CHUNK_F4];
            float yt[OGD_ROWS], ck[OGD_ROWS];
#pragma unroll
            for (int j = 0; j < OGD_ROWS; ++j) {
                const float* r = r0 + (int64_t)(k + j) * stride;
                ck[j] = coef[k + j];
#pragma unroll
                for (int u = 0; u < GEM_CHUNK_F4; ++u) {
                    const int q = threadIdx.x + u * CL_THREADS;
                    y[j][u] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (q < n4) y[j][u] = reinterpret_cast<const float4*>(r)[q];
                }
                yt[j] = tail < cnt ? r[tail] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < OGD_ROWS; ++j) {
#pragma unroll
                for (int u = 0; u < GEM_CHUNK_F4; ++u) {
                    h.X[u].x = sub_rn(h.X[u].x, mul_rn(ck[j], y[j][u].x));
                    h.X[u].y = sub_rn(h.X[u].y, mul_rn(ck[j], y[j][u].y));
                    h.X[u].z = sub_rn(h.X[u].z, mul_rn(ck[j], y[j][u].z));
                    h.X[u].w = sub_rn(h.X[u].w, mul_rn(ck[j], y[j][u].w));
                }
                h.xt = sub_rn(h.xt, mul_rn(ck[j], yt[j]));
            }
        }
        for (; k < nrows; ++k) {
            const float* r = r0 + (int64_t)k * stride;
            const float ck = coef[k];
#pragma unroll
            for (int u = 0; u < GEM_CHUNK_F4; ++u) {
                const int q = threadIdx.x + u * CL_THREADS;
                if (q < n4) {
                    const float4 y = reinterpret_cast<const float4*>(r)[q];
                    h.X[u].x = sub_rn(h.X[u].x, mul_rn(ck, y.x));
                    h.X[u].y = sub_rn(h.X[u].y, mul_rn(ck, y.y));
                    h.X[u].z = sub_rn(h.X[u].z, mul_rn(ck, y.z));
                    h.X[u].w = sub_rn(h.X[u].w, mul_rn(ck, y.w));
                }
            }
            if (tail < cnt) h.xt = sub_rn(h.xt, mul_rn(ck, r[tail]));
        }
#pragma unroll
        for (int u = 0; u < GEM_CHUNK_F4; ++u) {
            const int q = threadIdx.x + u * CL_THREADS;
            if (q < n4)
                reinterpret_cast<float4*>(dst + off)[q] = make_float4(mul_rn(h.X[u].x, alpha), mul_rn(h.X[u].y, alpha),
                                                                      mul_rn(h.X[u].z, alpha), mul_rn(h.X[u].w, alpha));
        }
        if (tail < cnt) dst[off + tail] = mul_rn(h.xt, alpha);
    }
}

// ---- the clip norm of the gradient a consumed_step consumes, from the step's own gradient functor.
// seg_activity_kernel<true>'s sum as the compiler emits it there, written out so that an un-projected step measures the norm
// ia_grad_norm measures bit for bit (tests/test_agem_gpu.py compares them): in the float4 body four separately rounded squares
// added left to right and then to the running sum, in the scalar tail one fma.
__device__ __forceinline__ float sumsq4_rn(float ss, const vecf<4>& x) {
#pragma clang fp contract(off)
    const float aa = x[0] * x[0], bb = x[1] * x[1], cc = x[2] * x[2], dd = x[3] * x[3];
    const float t = ((aa + bb) + cc) + dd;
    return ss + t;
}

// Not projecting: the raw sum of g^2 over every chunk, as ia_grad_norm's first pass.  Projecting: the sum of G^2, G the functor's
// gradient, over the chunks of live tensors; a dead tensor's chunk stores 0 (its .grad is None for torch's clip norm) and is not
// read.  seg_active is read only (NULL: every tensor live): the variant's dots kernel has set it.
// A gradient functor whose answer depends on the tensor (packed_grad: the tensor's kind) has for_segment(seg); every other one is
// used as it is.
template <class Grad, class = void> struct grad_per_segment : std::false_type {};
template <class Grad>
struct grad_per_segment<Grad, std::void_t<decltype(std::declval<const Grad&>().for_segment(0))>> : std::true_type {};

template <class Grad>
__device__ __forceinline__ decltype(auto) at_segment(const Grad& grad, int seg) {
    if constexpr (grad_per_segment<Grad>::value) return grad.for_segment(seg);
    else return (grad);
}

template <class Source>
__global__ __launch_bounds__(CL_THREADS) void consumed_norm_kernel(const float* __restrict__ g, const int4* __restrict__ table,
                                                                   int nchunks, const int* __restrict__ seg_active,
                                                                   const Source src, float grad_scale,
                                                                   float* __restrict__ chunk_sumsq) {
    __shared__ float sh[CL_THREADS / 64];
    const auto grad = src.begin();
    const bool projecting = grad.projecting();
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int4 e = table[c];
        const int off = e.x, cnt = e.y, n4 = cnt >> 2;
        float ss = 0.f;
        if (!projecting) {
            for (int q = threadIdx.x; q < n4; q += CL_THREADS) ss = sumsq4_rn(ss, ldv<4>(g, off + (q << 2)));
            for (int i = (n4 << 2) + threadIdx.x; i < cnt; i += CL_THREADS) ss = __builtin_fmaf(g[off + i], g[off + i], ss);
        } else if (!seg_active || seg_active[e.z]) {
            decltype(auto) seg_grad = at_segment(grad, e.z);     // workgroup-uniform
            for (int q = threadIdx.x; q < n4; q += CL_THREADS) {
                const int at = off + (q << 2);
                ss = sumsq4_rn(ss, seg_grad(ldv<4>(g, at), at, grad_scale));
            }
            for (int i = (n4 << 2) + threadIdx.x; i < cnt; i += CL_THREADS) {
                const float G = seg_grad(ldv<1>(g, off + i), off + i, grad_scale)[0];
                ss = __builtin_fmaf(G, G, ss);
            }
        }
        const float t = block_sum(ss, sh);
        if (threadIdx.x == 0) chunk_sumsq[c] = t;
    }
}

// ---- Piggyback (Mallya, Davis, Lazebnik 2018): a fixed backbone `base` and, per language, a binary mask over it that is
// trained through real-valued scores.  Per tensor a kind (workgroup-uniform per chunk, read inside the chunk loop as group_of is):
//   free    the plain rule on theta, so a free tensor moves as under the plain step
//   masked  ge = g * grad_scale [* coef];  gs = ge * base;  score, m, v = AdamW(score, gs) with weight decay 0 (decay factor 1);
//           theta = score >= threshold ? base : +0;  every product rounded on its own
//   frozen  nothing but the bf16 image
// A masked element moves 38 B (g, base, score, m, v in; score, m, v, theta and the bf16 image out), a free one 30 B.
constexpr int KIND_FREE = IA_MASK_FREE, KIND_MASKED = IA_MASK_MASKED, KIND_FROZEN = IA_MASK_FROZEN;   // anything else is free

struct score_rule {
    const float* base; float* scores; float threshold;
    static constexpr bool reads_theta = false;       // theta is an output only
    template <bool CLIP, int W>
    __device__ __forceinline__ void apply(vecf<W>& P, const vecf<W>& G, vecf<W>& M, vecf<W>& V, int64_t at,
                                          const chunk_consts& k) const {
        const vecf<W> B = ldv<W>(base, at);
        vecf<W> S = ldv<W>(scores, at);
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const float eff = eff_grad<CLIP>(mul_rn(G[j], k.grad_scale), k);
            adamw1_rn<W == 1>(S[j], mul_rn(eff, B[j]), M[j], V[j], 1.f, k);
            P[j] = S[j] >= threshold ? B[j] : 0.f;
        }
        stv<W>(scores, at, S);
    }
};

struct masked_step {
    const float* base; float* scores; const int* seg_kind; float threshold;
    __device__ __forceinline__ masked_step begin() const { return *this; }
    __device__ __forceinline__ score_rule kind_rule() const { return {base, scores, threshold}; }
};

// ---- PackNet (Mallya, Lazebnik 2018): all languages share theta, and one byte per weight says whose it is: 0 free, t >= 1 the
// t-th language's.  The kinds are Piggyback's, with `packed` in the masked slot:
//   packed  per element: owner == train_owner -> the plain rule (ge = g * grad_scale [* coef], the group's lr and weight decay);
//           otherwise theta and both moments keep their bit patterns.  The bf16 image follows theta for every element.
//   free    the plain rule;   frozen  nothing but the bf16 image
// A packed element moves 31 B (g, theta, m, v and the owner byte in; theta, m, v and the bf16 image out), one more than a free one.
__device__ __forceinline__ void ld_owner(const unsigned char* __restrict__ owner, int64_t at, unsigned char (&o)[4]) {
    const uchar4 q = *reinterpret_cast<const uchar4*>(owner + at);      // at is a multiple of 4 in a chunk's body
    o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
}
__device__ __forceinline__ void ld_owner(const unsigned char* __restrict__ owner, int64_t at, unsigned char (&o)[1]) {
    o[0] = owner[at];
}

struct owner_rule {
    const unsigned char* owner; int train_owner;
    static constexpr bool reads_theta = true;
    template <bool CLIP, int W>
    __device__ __forceinline__ void apply(vecf<W>& P, const vecf<W>& G, vecf<W>& M, vecf<W>& V, int64_t at,
                                          const chunk_consts& k) const {
        unsigned char o[W];
        ld_owner(owner, at, o);
#pragma unroll
        for (int j = 0; j < W; ++j)
            if ((int)o[j] == train_owner)
                adamw1_rn<W == 1>(P[j], eff_grad<CLIP>(mul_rn(G[j], k.grad_scale), k), M[j], V[j], k.decay, k);
    }
};

struct packed_step {
    const unsigned char* owner; const int* seg_kind; int train_owner;
    __device__ __forceinline__ packed_step begin() const { return *this; }
    __device__ __forceinline__ owner_rule kind_rule() const { return {owner, train_owner}; }
};

// ---- Kinds alone (the LoRA step, csrc/lora.hip): free tensors take the plain rule and every other tensor is left to the caller.
// seg_kind holds IA_MASK_FREE and IA_MASK_FROZEN only, so kind_rule() is never reached; it is the plain rule.
struct kinds_step {
    const int* seg_kind;
    __device__ __forceinline__ kinds_step begin() const { return *this; }
    __device__ __forceinline__ consumed_rule<scaled_grad> kind_rule() const { return {}; }
};

// A variant with per-tensor kinds has seg_kind and kind_rule(), the rule of its KIND_MASKED slot; its free tensors take the plain
// rule and its frozen ones are never written.
template <class Rule, class = void> struct has_kinds : std::false_type {};
template <class Rule>
struct has_kinds<Rule, std::void_t<decltype(std::declval<const Rule&>().kind_rule())>> : std::true_type {};

// The clip norm of the packed step: the raw gradient (the finisher scales the roots, as for ia_grad_norm) where the step consumes
// it, +0 elsewhere -- in a frozen tensor and where owner != train_owner in a packed one.
struct packed_grad {
    const unsigned char* owner; const int* seg_kind; int train_owner, kind;
    __device__ __forceinline__ bool projecting() const { return true; }      // never the raw sum over every chunk
    __device__ __forceinline__ packed_grad for_segment(int seg) const { return {owner, seg_kind, train_owner, seg_kind[seg]}; }
    template <int W>
    __device__ __forceinline__ vecf<W> operator()(const vecf<W>& G, int64_t at, float) const {
        vecf<W> a = G;
        if (kind == KIND_FROZEN) {
#pragma unroll
            for (int j = 0; j < W; ++j) a[j] = 0.f;
        } else if (kind == KIND_MASKED) {
            unsigned char o[W];
            ld_owner(owner, at, o);
#pragma unroll
            for (int j = 0; j < W; ++j) a[j] = (int)o[j] == train_owner ? G[j] : 0.f;
        }
        return a;
    }
};

struct packed_source {
    const unsigned char* owner; const int* seg_kind; int train_owner;
    __device__ __forceinline__ packed_grad begin() const { return {owner, seg_kind, train_owner, KIND_FREE}; }
};

// ---- the chunk walker.  One access of W elements: the common operands in, the variant's rule, the common operands out.
template <bool CLIP, int W, class Rule>
__device__ __forceinline__ void step_vec(const Rule& rule, float* __restrict__ p, const float* __restrict__ g,
                                         float* __restrict__ m, float* __restrict__ v,
                                         unsigned short* __restrict__ shadow_bf16, int at, const chunk_consts& k) {
    vecf<W> P;
    if constexpr (Rule::reads_theta) P = ldv<W>(p, at);
    const vecf<W> G = ldv<W>(g, at);
    vecf<W> M = ldv<W>(m, at), V = ldv<W>(v, at);
    rule.template apply<CLIP, W>(P, G, M, V, at, k);
    stv<W>(p, at, P);
    stv<W>(m, at, M);
    stv<W>(v, at, V);
    if (shadow_bf16) {
        if constexpr (W == 4) *reinterpret_cast<ushort4*>(shadow_bf16 + at) = bf16_bits(make_float4(P[0], P[1], P[2], P[3]));
        else shadow_bf16[at] = bf16_bits(P[0]);
    }
}

// One live chunk under one rule: the float4 body and the scalar tail, split at cnt >> 2
template <bool CLIP, class Rule>
__device__ __forceinline__ void walk_chunk(const Rule& rule, float* __restrict__ p, const float* __restrict__ g,
                                           float* __restrict__ m, float* __restrict__ v,
                                           unsigned short* __restrict__ shadow_bf16, int off, int cnt, const chunk_consts& k) {
    const int n4 = cnt >> 2;
    for (int q = threadIdx.x; q < n4; q += CL_THREADS) step_vec<CLIP, 4>(rule, p, g, m, v, shadow_bf16, off + (q << 2), k);
    for (int i = (n4 << 2) + threadIdx.x; i < cnt; i += CL_THREADS) step_vec<CLIP, 1>(rule, p, g, m, v, shadow_bf16, off + i, k);
}

// The segmented AdamW of every variant.  CLIP: norm_state = {norm, coef, non-finite flag, max_norm} is read from the device; when
// the flag is set and skip_nonfinite is given the launch writes nothing at all.
template <bool CLIP, class Variant>
__global__ __launch_bounds__(CL_THREADS) void adamw_seg_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                               float* __restrict__ m, float* __restrict__ v,
                                                               const int4* __restrict__ table, int nchunks,
                                                               const int* __restrict__ seg_active,
                                                               const int* __restrict__ seg_step, const group_table groups,
                                                               const int* __restrict__ seg_group, float b1, float b2, float eps,
                                                               float grad_scale, unsigned short* __restrict__ shadow_bf16,
                                                               const float* __restrict__ norm_state, int skip_nonfinite,
                                                               const Variant variant) {
    __shared__ float sh_c[2];
    float coef = 1.f;
    if (CLIP) {
        if (skip_nonfinite && norm_state[2] != 0.f) return;
        coef = norm_state[1];
    }
    // The variant's launch-uniform state (violated, alpha, K and v).  begin() may contain a barrier (gem_source fills shared
    // memory): it has to stay in control flow that is uniform over the workgroup, as it is after the launch-uniform return above.
    const auto rule = variant.begin();
    using Rule = std::remove_cv_t<decltype(rule)>;
    constexpr bool KINDS = has_kinds<Rule>::value;               // masked_step, packed_step: per-tensor kinds
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int4 e = table[c];           // x = offset (multiple of 4), y = count, z = segment id
        int kind = KIND_FREE;                                    // workgroup-uniform
        if constexpr (KINDS) kind = rule.seg_kind[e.z];
        if (kind == KIND_FROZEN || !seg_active[e.z]) {           // never written / no gradient: only the bf16 image is kept in step
            if (shadow_bf16)
                for (int i = threadIdx.x; i < e.y; i += CL_THREADS) shadow_bf16[e.x + i] = bf16_bits(p[e.x + i]);
            continue;
        }
        const int gi = group_of(seg_group, e.z, groups.n);      // workgroup-uniform
        const float lr = groups.lr[gi], wd = groups.weight_decay[gi];
        __syncthreads();
        if (threadIdx.x == 0) {
            const double step = (double)(seg_step[e.z] + 1);
            sh_c[0] = (float)((double)lr / (1.0 - pow((double)b1, step)));
            sh_c[1] = (float)(1.0 / sqrt(1.0 - pow((double)b2, step)));
        }
        __syncthreads();
        const chunk_consts k = {__builtin_fmaf(-lr, wd, 1.f), 1.f - b1, b2, 1.f - b2, eps, sh_c[0], sh_c[1], grad_scale, coef};
        if constexpr (KINDS) {
            if (kind == KIND_MASKED)
                walk_chunk<CLIP>(rule.kind_rule(), p, g, m, v, shadow_bf16, e.x, e.y, k);
            else
                walk_chunk<CLIP>(consumed_rule<scaled_grad>{}, p, g, m, v, shadow_bf16, e.x, e.y, k);
        } else {
            walk_chunk<CLIP>(rule, p, g, m, v, shadow_bf16, e.x, e.y, k);
        }
    }
}

// After a step: a live tensor's counter moves unless the step was skipped or the tensor is frozen, and every flag is cleared.
// counters = {clipped steps, skipped steps}, with norm_state or both NULL (nothing measured).  projected (proj_state + 3 or
// gem_state + GEM_VIOLATED) with its counter: a skipped step is not counted as projected.  solved (gem_state + GEM_SOLVED) with
// its counter: an unsolved program is counted whether or not the step was skipped.  Each of the three and seg_kind may be NULL.
__global__ void seg_step_advance_kernel(int* __restrict__ seg_active, int* __restrict__ seg_step, int nseg,
                                        const float* __restrict__ norm_state, int skip_nonfinite, int* __restrict__ counters,
                                        const float* __restrict__ projected, int* __restrict__ projected_count,
                                        const float* __restrict__ solved, int* __restrict__ unsolved_count,
                                        const int* __restrict__ seg_kind) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    const bool skipped = norm_state && skip_nonfinite && norm_state[2] != 0.f;
    if (s < nseg) {
        const bool frozen = seg_kind && seg_kind[s] == KIND_FROZEN;
        seg_step[s] += (!skipped && seg_active[s] && !frozen) ? 1 : 0;
        seg_active[s] = 0;
    }
    if (s == 0) {
        if (skipped) counters[1] += 1;
        else if (norm_state && norm_state[1] < 1.f) counters[0] += 1;
        if (projected && !skipped && projected[0] != 0.f) projected_count[0] += 1;
        if (solved && solved[0] == 0.f) unsolved_count[0] += 1;
    }
}

// Scores -> bits.  A chunk starts on a 64-float boundary of the flat buffer and holds at most 4096 elements = 64 words; wave w of
// the workgroup takes words w, w + 4, ... (a wave-uniform trip count), lane i votes for element 64 * j + i and the 64-bit ballot IS
// word j.  Lanes past the chunk's count and every lane of a tensor that is not masked vote 0, so gaps and other tensors read 0.
__global__ __launch_bounds__(CL_THREADS) void mask_pack_kernel(const float* __restrict__ scores, const int4* __restrict__ table,
                                                               int nchunks, const int* __restrict__ seg_kind, float threshold,
                                                               unsigned long long* __restrict__ bits, int64_t nwords,
                                                               int* __restrict__ seg_kept) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int4 e = table[c];
        const int off = e.x, cnt = e.y, words = (cnt + 63) >> 6;
        const bool masked = seg_kind[e.z] == KIND_MASKED;        // workgroup-uniform
        const int64_t word0 = (int64_t)(off >> 6);
        int kept = 0;
        for (int j = wave; j < words; j += CL_THREADS / 64) {
            const int i = (j << 6) + lane;
            const bool on = masked && i < cnt && scores[off + i] >= threshold;
            const unsigned long long word = __ballot(on);
            if (lane == 0 && word0 + j < nwords) bits[word0 + j] = word;
            kept += __popcll(word);
        }
        if (seg_kept && lane == 0 && kept) atomicAdd(seg_kept + e.z, kept);
    }
}

// Bits -> weights: theta = bit ? base : +0 inside masked tensors; the bf16 image of every tensor follows theta.
__global__ __launch_bounds__(CL_THREADS) void mask_apply_kernel(float* __restrict__ p, const float* __restrict__ base,
                                                                const unsigned long long* __restrict__ bits, int64_t nwords,
                                                                const int4* __restrict__ table, int nchunks,
                                                                const int* __restrict__ seg_kind,
                                                                unsigned short* __restrict__ shadow_bf16) {
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int4 e = table[c];
        const int off = e.x, cnt = e.y, n4 = cnt >> 2;
        const bool masked = seg_kind[e.z] == KIND_MASKED;        // workgroup-uniform
        if (!masked && !shadow_bf16) continue;
        const int64_t word0 = (int64_t)(off >> 6);
        for (int q = threadIdx.x; q < n4; q += CL_THREADS) {
            float4 P;
            if (masked) {
                const int64_t wi = word0 + (q >> 4);             // 16 float4 per word
                const unsigned long long word = wi < nwords ? bits[wi] : 0ull;
                const unsigned nib = (unsigned)(word >> ((q & 15) << 2)) & 15u;
                const float4 B = reinterpret_cast<const float4*>(base + off)[q];
                P = make_float4(nib & 1u ? B.x : 0.f, nib & 2u ? B.y : 0.f, nib & 4u ? B.z : 0.f, nib & 8u ? B.w : 0.f);
                reinterpret_cast<float4*>(p + off)[q] = P;
            } else {
                P = reinterpret_cast<const float4*>(p + off)[q];
            }
            if (shadow_bf16) reinterpret_cast<ushort4*>(shadow_bf16 + off)[q] = bf16_bits(P);
        }
        for (int i = (n4 << 2) + threadIdx.x; i < cnt; i += CL_THREADS) {
            float P;
            if (masked) {
                const int64_t wi = word0 + (i >> 6);
                const unsigned long long word = wi < nwords ? bits[wi] : 0ull;
                P = (word >> (i & 63)) & 1ull ? base[off + i] : 0.f;
                p[off + i] = P;
            } else {
                P = p[off + i];
            }
            if (shadow_bf16) shadow_bf16[off + i] = bf16_bits(P);
        }
    }
}

// ---- PackNet's pruning: per packed tensor, the r-th smallest |theta| among its free elements (owner == 0), r = floor(fraction * n),
// by an exact radix select on the 31-bit pattern of |theta| (the order of finite magnitudes), most significant digit first:
//   pack_hist_kernel    one pass per digit (8, 8, 8 and 7 bits).  A workgroup counts the digit of the free elements whose higher
//                       digits equal the tensor's prefix into a histogram in LDS and adds it to hist[seg][bin] with integer
//                       atomics: the sums do not depend on the order of arrival.  With more than 2048 chunks a workgroup visits
//                       chunks of different tensors, so the histogram is flushed whenever the tensor changes, and at the end.
//                       Only elements below a chunk's count are read: never a float4 over a short tail, never an alignment gap.
//   pack_pick_kernel    one workgroup per tensor: the first pass fixes n (the histogram's total) and r; every pass picks the bin
//                       that holds the rank, extends the prefix, reduces the rank to one inside that bin and clears the histogram.
//                       The last pass also knows the counts: released = the free elements at or below the cutoff = r - rank +
//                       the bin's inclusive sum, newly owned = n - released; no pass over the data counts them.
//   pack_prune_kernel   free elements at or below the cutoff are released (theta = +0, owner stays 0), the other free ones get
//                       owner = task; both moments of every element of a packed tensor become +0; the bf16 image of every tensor
//                       is rewritten.
constexpr int PK_BINS = 256, PK_PASSES = 4;
static_assert(PK_BINS == CL_THREADS, "one histogram bin per thread");
__host__ __device__ constexpr int pk_shift(int pass) { return pass == 0 ? 23 : pass == 1 ? 15 : pass == 2 ? 7 : 0; }
__host__ __device__ constexpr int pk_width(int pass) { return pass == 3 ? 7 : 8; }

struct alignas(16) pack_sel {     // per tensor, in the workspace (zeroed by the host before the first pass)
    unsigned prefix;              // the digits chosen so far, in place; after the last pass the cutoff's pattern
    unsigned rank;                // 1-based rank of the cutoff among the elements that share the prefix
    unsigned r;                   // floor(fraction * n); 0: nothing is released
    unsigned n;                   // free elements of the tensor
};

__device__ __forceinline__ void pk_flush(unsigned* sh, unsigned* __restrict__ hist, int seg) {
    __syncthreads();
    const unsigned h = sh[threadIdx.x];
    if (h) atomicAdd(hist + (int64_t)seg * PK_BINS + threadIdx.x, h);
    sh[threadIdx.x] = 0;
    __syncthreads();
}

__global__ __launch_bounds__(CL_THREADS) void pack_hist_kernel(const float* __restrict__ p, const unsigned char* __restrict__ owner,
                                                               const int4* __restrict__ table, int nchunks,
                                                               const int* __restrict__ seg_kind, const pack_sel* __restrict__ sel,
                                                               int pass, unsigned* __restrict__ hist) {
    __shared__ unsigned sh[PK_BINS];
    sh[threadIdx.x] = 0;
    __syncthreads();
    const int shift = pk_shift(pass), up = shift + pk_width(pass);      // up == 31 in the first pass: every pattern matches
    const unsigned digit_mask = (1u << pk_width(pass)) - 1u;
    int cur = -1;                                                        // the tensor the LDS histogram belongs to
    unsigned prefix_up = 0;
    bool counted = true;                                                 // false: r == 0, nothing to select in this tensor
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int4 e = table[c];
        if (seg_kind[e.z] != KIND_MASKED) continue;                      // workgroup-uniform, as everything up to the counting
        if (e.z != cur) {
            if (cur >= 0) pk_flush(sh, hist, cur);
            cur = e.z;
            if (pass > 0) {
                const pack_sel s = sel[e.z];
                prefix_up = s.prefix >> up;
                counted = s.r != 0;
            }
        }
        if (!counted) continue;
        const int off = e.x, cnt = e.y, n4 = cnt >> 2;
        for (int q = threadIdx.x; q < n4; q += CL_THREADS) {
            const uint4 x = reinterpret_cast<const uint4*>(p + off)[q];
            const uchar4 o = reinterpret_cast<const uchar4*>(owner + off)[q];
            const unsigned k0 = x.x & 0x7FFFFFFFu, k1 = x.y & 0x7FFFFFFFu, k2 = x.z & 0x7FFFFFFFu, k3 = x.w & 0x7FFFFFFFu;
            if (o.x == 0 && k0 >> up == prefix_up) atomicAdd(sh + ((k0 >> shift) & digit_mask), 1u);
            if (o.y == 0 && k1 >> up == prefix_up) atomicAdd(sh + ((k1 >> shift) & digit_mask), 1u);
            if (o.z == 0 && k2 >> up == prefix_up) atomicAdd(sh + ((k2 >> shift) & digit_mask), 1u);
            if (o.w == 0 && k3 >> up == prefix_up) atomicAdd(sh + ((k3 >> shift) & digit_mask), 1u);
        }
        for (int i = (n4 << 2) + threadIdx.x; i < cnt; i += CL_THREADS) {
            const unsigned k = __float_as_uint(p[off + i]) & 0x7FFFFFFFu;
            if (owner[off + i] == 0 && k >> up == prefix_up) atomicAdd(sh + ((k >> shift) & digit_mask), 1u);
        }
    }
    if (cur >= 0) pk_flush(sh, hist, cur);
}

__global__ __launch_bounds__(PK_BINS) void pack_pick_kernel(unsigned* __restrict__ hist, pack_sel* __restrict__ sel,
                                                            const int* __restrict__ seg_kind, int pass, float fraction,
                                                            int* __restrict__ seg_counts) {
    __shared__ unsigned sc[PK_BINS];
    const int seg = blockIdx.x, t = threadIdx.x;
    if (seg_kind[seg] != KIND_MASKED) return;
    const pack_sel s = sel[seg];
    if (pass > 0 && !s.r) return;                                        // workgroup-uniform
    const unsigned h = hist[(int64_t)seg * PK_BINS + t];
    hist[(int64_t)seg * PK_BINS + t] = 0;                                // for the next pass
    sc[t] = h;
    __syncthreads();
    for (int d = 1; d < PK_BINS; d <<= 1) {                              // inclusive scan
        const unsigned a = t >= d ? sc[t - d] : 0u;
        __syncthreads();
        sc[t] += a;
        __syncthreads();
    }
    const unsigned incl = sc[t], excl = incl - h;
    unsigned rank = s.rank, r = s.r, n = s.n;
    if (pass == 0) {
        n = sc[PK_BINS - 1];
        rank = r = (unsigned)floor((double)fraction * (double)n);        // fraction < 1, so r < n
        if (r == 0) {
            if (t == 0) {
                sel[seg] = {0u, 0u, 0u, n};
                seg_counts[2 * seg] = 0;
                seg_counts[2 * seg + 1] = (int)n;                        // everything free is taken
            }
            return;
        }
    }
    if (h && excl < rank && rank <= incl) {                              // one thread
        sel[seg] = {s.prefix | ((unsigned)t << pk_shift(pass)), rank - excl, r, n};
        if (pass == PK_PASSES - 1) {
            const unsigned released = r - rank + incl;                   // r - rank lie below the prefix, incl at or below the cutoff
            seg_counts[2 * seg] = (int)released;
            seg_counts[2 * seg + 1] = (int)(n - released);
        }
    }
}

// One element: a free one is released, or taken by `task`
__device__ __forceinline__ void pk_release(float& P, unsigned char& o, bool active, unsigned cutoff, unsigned char task) {
    if (o != 0) return;
    if (active && (__float_as_uint(P) & 0x7FFFFFFFu) <= cutoff) P = 0.f;
    else o = task;
}

__global__ __launch_bounds__(CL_THREADS) void pack_prune_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                                unsigned char* __restrict__ owner, const int4* __restrict__ table,
                                                                int nchunks, const int* __restrict__ seg_kind,
                                                                const pack_sel* __restrict__ sel, int task,
                                                                unsigned short* __restrict__ shadow_bf16) {
    const unsigned char mine = (unsigned char)task;
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int4 e = table[c];
        const int off = e.x, cnt = e.y, n4 = cnt >> 2;
        if (seg_kind[e.z] != KIND_MASKED) {                              // workgroup-uniform: only the bf16 image
            if (shadow_bf16)
                for (int i = threadIdx.x; i < cnt; i += CL_THREADS) shadow_bf16[off + i] = bf16_bits(p[off + i]);
            continue;
        }
        const pack_sel s = sel[e.z];
        const bool active = s.r != 0;
        const unsigned cutoff = s.prefix;
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int q = threadIdx.x; q < n4; q += CL_THREADS) {
            float4 P = reinterpret_cast<float4*>(p + off)[q];
            uchar4 o = reinterpret_cast<uchar4*>(owner + off)[q];
            pk_release(P.x, o.x, active, cutoff, mine);
            pk_release(P.y, o.y, active, cutoff, mine);
            pk_release(P.z, o.z, active, cutoff, mine);
            pk_release(P.w, o.w, active, cutoff, mine);
            reinterpret_cast<float4*>(p + off)[q] = P;
            reinterpret_cast<uchar4*>(owner + off)[q] = o;
            reinterpret_cast<float4*>(m + off)[q] = zero;
            reinterpret_cast<float4*>(v + off)[q] = zero;
            if (shadow_bf16) reinterpret_cast<ushort4*>(shadow_bf16 + off)[q] = bf16_bits(P);
        }
        for (int i = (n4 << 2) + threadIdx.x; i < cnt; i += CL_THREADS) {
            float P = p[off + i];
            unsigned char o = owner[off + i];
            pk_release(P, o, active, cutoff, mine);
            p[off + i] = P;
            owner[off + i] = o;
            m[off + i] = 0.f;
            v[off + i] = 0.f;
            if (shadow_bf16) shadow_bf16[off + i] = bf16_bits(P);
        }
    }
}

// Owner map -> weights: theta = lo <= owner <= hi ? base : +0 inside packed tensors; the bf16 image of every tensor follows theta.
__global__ __launch_bounds__(CL_THREADS) void pack_apply_kernel(float* __restrict__ p, const float* __restrict__ base,
                                                                const unsigned char* __restrict__ owner,
                                                                const int4* __restrict__ table, int nchunks,
                                                                const int* __restrict__ seg_kind, int lo, int hi,
                                                                unsigned short* __restrict__ shadow_bf16) {
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int4 e = table[c];
        const int off = e.x, cnt = e.y, n4 = cnt >> 2;
        const bool packed = seg_kind[e.z] == KIND_MASKED;        // workgroup-uniform
        if (!packed && !shadow_bf16) continue;
        for (int q = threadIdx.x; q < n4; q += CL_THREADS) {
            float4 P;
            if (packed) {
                const float4 B = reinterpret_cast<const float4*>(base + off)[q];
                const uchar4 o = reinterpret_cast<const uchar4*>(owner + off)[q];
                P = make_float4(lo <= o.x && o.x <= hi ? B.x : 0.f, lo <= o.y && o.y <= hi ? B.y : 0.f,
                                lo <= o.z && o.z <= hi ? B.z : 0.f, lo <= o.w && o.w <= hi ? B.w : 0.f);
                reinterpret_cast<float4*>(p + off)[q] = P;
            } else {
                P = reinterpret_cast<const float4*>(p + off)[q];
            }
            if (shadow_bf16) reinterpret_cast<ushort4*>(shadow_bf16 + off)[q] = bf16_bits(P);
        }
        for (int i = (n4 << 2) + threadIdx.x; i < cnt; i += CL_THREADS) {
            float P;
            if (packed) {
                const int o = owner[off + i];
                P = lo <= o && o <= hi ? base[off + i] : 0.f;
                p[off + i] = P;
            } else {
                P = p[off + i];
            }
            if (shadow_bf16) shadow_bf16[off + i] = bf16_bits(P);
        }
    }
}

inline int cap_grid(int64_t work_items, int per_block) {
    int64_t b = (work_items + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

inline int chunk_grid(int nchunks) { return nchunks < 2048 ? nchunks : 2048; }

inline bool groups_ok(const int32_t* seg_group, int ngroups, const float* group_lr, const float* group_weight_decay) {
    return ngroups >= 1 && ngroups <= IA_MAX_PARAM_GROUPS && group_lr && group_weight_decay && (ngroups == 1 || seg_group) &&
           (!seg_group || ia_is_aligned(seg_group, 4));
}

inline group_table make_group_table(int ngroups, const float* group_lr, const float* group_weight_decay) {
    group_table t = {};
    t.n = ngroups;
    for (int k = 0; k < ngroups; ++k) { t.lr[k] = group_lr[k]; t.weight_decay[k] = group_weight_decay[k]; }
    return t;
}

inline group_table one_group(float lr, float weight_decay) { return make_group_table(1, &lr, &weight_decay); }

// The operands every segmented step shares.  seg_group NULL: every tensor in group 0.  norm_state and counters: both (the clip
// coefficient and the non-finite flag are read from the device) or neither.
struct step_head {
    float *theta; const float* grad; float *exp_avg, *exp_avg_sq;
    const int4* table; int nchunks; int32_t *seg_active, *seg_step; int nseg, all_active;
    float b1, b2, eps, grad_scale; unsigned short* shadow;
    const int32_t* seg_group; const float* norm_state; int skip_nonfinite; int32_t* counters;
};

inline step_head make_head(float* theta, const float* grad, float* exp_avg, float* exp_avg_sq, const int32_t* chunk_table,
                           int nchunks, int32_t* seg_active, int32_t* seg_step, int nseg, int all_active, float beta1, float beta2,
                           float eps, float grad_scale, void* shadow_bf16, const int32_t* seg_group, const float* norm_state,
                           int skip_nonfinite, int32_t* counters) {
    return {theta, grad, exp_avg, exp_avg_sq, (const int4*)chunk_table, nchunks, seg_active, seg_step, nseg, all_active,
            beta1, beta2, eps, grad_scale, (unsigned short*)shadow_bf16, seg_group, norm_state, skip_nonfinite, counters};
}

inline bool head_ok(const step_head& h) {
    if (!h.theta || !h.grad || !h.exp_avg || !h.exp_avg_sq || !h.table || !h.seg_active || !h.seg_step || h.nchunks <= 0 ||
        h.nseg <= 0 || (h.norm_state == nullptr) != (h.counters == nullptr))
        return false;
    return ia_is_aligned(h.theta, 16) && ia_is_aligned(h.grad, 16) && ia_is_aligned(h.exp_avg, 16) &&
           ia_is_aligned(h.exp_avg_sq, 16) && ia_is_aligned(h.table, 16) && (!h.shadow || ia_is_aligned(h.shadow, 8));
}

inline bool si_operands_ok(const float* path_w, const float* omega, const float* theta_star) {
    if (!path_w || (omega == nullptr) != (theta_star == nullptr)) return false;
    return ia_is_aligned(path_w, 16) && (!omega || (ia_is_aligned(omega, 16) && ia_is_aligned(theta_star, 16)));
}

inline bool rwalk_operands_ok(const float* fisher, const float* path_w, const float* anchor, const float* score,
                              const float* importance, const float* theta_star) {
    const bool scores = path_w || anchor || score;
    if (!fisher || (scores && (!path_w || !anchor || !score)) || (importance == nullptr) != (theta_star == nullptr)) return false;
    return ia_is_aligned(fisher, 16) && (!scores || (ia_is_aligned(path_w, 16) && ia_is_aligned(anchor, 16) &&
                                                     ia_is_aligned(score, 16))) &&
           (!importance || (ia_is_aligned(importance, 16) && ia_is_aligned(theta_star, 16)));
}

inline bool proj_operands_ok(const float* ref, const float* proj_state, const int32_t* proj_counters) {
    if (!ref || !proj_state || !proj_counters) return false;
    return ia_is_aligned(ref, 16) && ia_is_aligned(proj_state, 4) && ia_is_aligned(proj_counters, 4);
}

inline bool gem_operands_ok(const float* refs, int64_t stride, int ntasks, const float* gem_state) {
    if (!refs || !gem_state || ntasks < 1 || ntasks > GEM_MAX || stride <= 0 || (stride & 3)) return false;
    return ia_is_aligned(refs, 16) && ia_is_aligned(gem_state, 4);
}

// What the host and the advance kernel need to know of a variant beyond its kernel operands
struct step_extras {
    bool flags_preset;       // the variant's dots kernel has set seg_active from the task gradient: never an activity pass here
    const float* projected; int32_t* projected_count; const float* solved; int32_t* unsolved_count;
    const int32_t* seg_kind;  // the masked and packed steps: the SAME array as the variant's seg_kind, so that walker and advance agree
    bool free_only;           // kinds_step: only free tensors are ever looked at, so the liveness pass skips the chunks of the others
};

// Every segmented step: liveness, the walker, the advance.  Arguments are validated by the callers.  Liveness: all_active marks
// every tensor; otherwise the flags are those of ia_grad_norm's first pass (norm_state given) or of the variant's dots kernel,
// or an activity pass over the gradient runs here.
template <class Variant>
int run_step(const step_head& h, const group_table& gt, const Variant& variant, const step_extras& x, hipStream_t st) {
    if (h.all_active) {    // 0x01010101: non-zero
        if (hipMemsetAsync(h.seg_active, 1, (size_t)h.nseg * sizeof(int32_t), st) != hipSuccess) return IA_LAUNCH_FAILED;
    } else if (!h.norm_state && !x.flags_preset) {
        hipLaunchKernelGGL(seg_activity_kernel<false>, dim3(chunk_grid(h.nchunks)), dim3(CL_THREADS), 0, st, h.grad, h.table,
                           h.nchunks, h.seg_active, (float*)nullptr, x.free_only ? x.seg_kind : (const int32_t*)nullptr);
    }
    auto kernel = h.norm_state ? adamw_seg_kernel<true, Variant> : adamw_seg_kernel<false, Variant>;
    hipLaunchKernelGGL(kernel, dim3(chunk_grid(h.nchunks)), dim3(CL_THREADS), 0, st, h.theta, h.grad, h.exp_avg, h.exp_avg_sq,
                       h.table, h.nchunks, h.seg_active, h.seg_step, gt, h.seg_group, h.b1, h.b2, h.eps, h.grad_scale, h.shadow,
                       h.norm_state, h.skip_nonfinite, variant);
    hipLaunchKernelGGL(seg_step_advance_kernel, dim3((h.nseg + 255) / 256), dim3(256), 0, st, h.seg_active, h.seg_step, h.nseg,
                       h.norm_state, h.skip_nonfinite, h.counters, x.projected, x.projected_count, x.solved, x.unsolved_count,
                       x.seg_kind);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}

int run_step_si(const step_head& h, const group_table& gt, float* path_w, const float* omega, const float* theta_star,
                float penalty_coef, hipStream_t st) {
    const float c2 = 2.f * penalty_coef;
    return omega ? run_step(h, gt, si_step<true>{path_w, omega, theta_star, c2}, step_extras{}, st)
                 : run_step(h, gt, si_step<false>{path_w, omega, theta_star, c2}, step_extras{}, st);
}

int run_step_agem(const step_head& h, const group_table& gt, const float* ref, const float* proj_state, int32_t* proj_counters,
                  hipStream_t st) {
    step_extras x = {};
    x.flags_preset = true;
    x.projected = proj_state + 3;
    x.projected_count = proj_counters;
    return run_step(h, gt, agem_step{{ref, proj_state}}, x, st);
}

// The clip norm of ia_grad_norm_projected / ia_grad_norm_gem: chunk sums of the consumed gradient, then the finisher, which
// leaves the root unscaled when the step projects (`projected` set on the device)
inline bool norm_operands_ok(const float* grad, const int32_t* chunk_table, int nchunks, const int32_t* seg_chunk_begin, int nseg,
                             const float* seg_norm, const float* norm_state, const void* workspace) {
    if (!grad || !chunk_table || !seg_chunk_begin || !seg_norm || !norm_state || !workspace || nchunks <= 0 || nseg <= 0)
        return false;
    return ia_is_aligned(grad, 16) && ia_is_aligned(chunk_table, 16) && ia_is_aligned(workspace, 4);
}

template <class Source>
int run_consumed_norm(const float* grad, const int32_t* chunk_table, int nchunks, const int32_t* seg_chunk_begin, int nseg,
                      float grad_scale, float max_norm, const int32_t* seg_active, float* seg_norm, float* norm_state,
                      void* workspace, const Source& src, const float* projected, hipStream_t st) {
    hipLaunchKernelGGL(consumed_norm_kernel<Source>, dim3(chunk_grid(nchunks)), dim3(CL_THREADS), 0, st, grad,
                       (const int4*)chunk_table, nchunks, seg_active, src, grad_scale, (float*)workspace);
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(GN_THREADS), 0, st, (const float*)workspace, seg_chunk_begin, nseg,
                       fabsf(grad_scale), max_norm, seg_norm, norm_state, projected);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}
}  // namespace

extern "C" int ia_cl_chunk_elems(void) { return CL_CHUNK; }

extern "C" int ia_cl_penalty(const float* theta, const float* theta_star, const float* weight, float coef, float* grad,
                             int accumulate, const int32_t* chunk_table, int nchunks, const float* seg_inv_numel,
                             float* seg_abs_mean, float* penalty_sum, ia_stream_t stream) {
    if (!theta || !theta_star || !weight || !chunk_table || nchunks <= 0) return IA_INVALID_VALUE;
    if (seg_abs_mean && !seg_inv_numel) return IA_INVALID_VALUE;
    if (!ia_is_aligned(theta, 16) || !ia_is_aligned(theta_star, 16) || !ia_is_aligned(weight, 16) ||
        (grad && !ia_is_aligned(grad, 16)) || !ia_is_aligned(chunk_table, 16))
        return IA_INVALID_VALUE;
    hipLaunchKernelGGL(cl_penalty_kernel, dim3(nchunks < 2048 ? nchunks : 2048), dim3(CL_THREADS), 0, (hipStream_t)stream,
                       theta, theta_star, weight, coef, grad, accumulate, (const int4*)chunk_table, nchunks,
                       seg_inv_numel, seg_abs_mean, penalty_sum);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}

extern "C" int ia_cl_fisher_accumulate(float* fisher, const float* grad, const float* loss_scalar, int64_t n,
                                       ia_stream_t stream) {
    if (!fisher || !grad || !loss_scalar || n <= 0 || !ia_is_aligned(fisher, 16) || !ia_is_aligned(grad, 16))
        return IA_INVALID_VALUE;
    hipLaunchKernelGGL((cl_accumulate_kernel<0>), dim3(cap_grid(n >> 2, CL_THREADS * 4)), dim3(CL_THREADS), 0,
                       (hipStream_t)stream, fisher, grad, loss_scalar, n);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}

extern "C" int ia_cl_abs_accumulate(float* omega, const float* grad, int64_t n, ia_stream_t stream) {
    if (!omega || !grad || n <= 0 || !ia_is_aligned(omega, 16) || !ia_is_aligned(grad, 16)) return IA_INVALID_VALUE;
    hipLaunchKernelGGL((cl_accumulate_kernel<1>), dim3(cap_grid(n >> 2, CL_THREADS * 4)), dim3(CL_THREADS), 0,
                       (hipStream_t)stream, omega, grad, (const float*)nullptr, n);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}

extern "C" int ia_adamw_step(float* theta, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                             float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                             void* shadow_bf16, ia_stream_t stream) {
    if (!theta || !grad || !exp_avg || !exp_avg_sq || n <= 0 || step < 1) return IA_INVALID_VALUE;
    if (!ia_is_aligned(theta, 16) || !ia_is_aligned(grad, 16) || !ia_is_aligned(exp_avg, 16) ||
        !ia_is_aligned(exp_avg_sq, 16) || (shadow_bf16 && !ia_is_aligned(shadow_bf16, 8)))
        return IA_INVALID_VALUE;
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    const float step_size = (float)(lr / bc1), inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
    hipLaunchKernelGGL(adamw_kernel, dim3(cap_grid(n >> 2, CL_THREADS * 4)), dim3(CL_THREADS), 0, (hipStream_t)stream, theta,
                       grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step_size, inv_bc2_sqrt,
                       grad_scale, (unsigned short*)shadow_bf16);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}

extern "C" int ia_adamw_step_segmented(float* theta, const float* grad, float* exp_avg, float* exp_avg_sq,
                                       const int32_t* chunk_table, int nchunks, int32_t* seg_active, int32_t* seg_step, int nseg,
                                       int all_active, float lr, float beta1, float beta2, float eps, float weight_decay,
                                       float grad_scale, void* shadow_bf16, ia_stream_t stream) {
    const step_head h = make_head(theta, grad, exp_avg, exp_avg_sq, chunk_table, nchunks, seg_active, seg_step, nseg, all_active,
                                  beta1, beta2, eps, grad_scale, shadow_bf16, nullptr, nullptr, 0, nullptr);
    if (!head_ok(h)) return IA_INVALID_VALUE;
    return run_step(h, one_group(lr, weight_decay), plain_step{}, step_extras{}, (hipStream_t)stream);
}

extern "C" size_t ia_grad_norm_workspace_bytes(int nchunks) { return nchunks > 0 ? (size_t)nchunks * sizeof(float) : 0; }

extern "C" int ia_grad_norm(const float* grad, const int32_t* chunk_table, int nchunks, const int32_t* seg_chunk_begin, int nseg,
                            float grad_scale, float max_norm, int32_t* seg_active, float* seg_norm, float* norm_state,
                            void* workspace, size_t workspace_bytes, ia_stream_t stream) {
    if (!norm_operands_ok(grad, chunk_table, nchunks, seg_chunk_begin, nseg, seg_norm, norm_state, workspace))
        return IA_INVALID_VALUE;
    if (workspace_bytes < ia_grad_norm_workspace_bytes(nchunks)) return IA_WORKSPACE_TOO_SMALL;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(seg_activity_kernel<true>, dim3(chunk_grid(nchunks)), dim3(CL_THREADS), 0, st, grad,
                       (const int4*)chunk_table, nchunks, seg_active, (float*)workspace, (const int32_t*)nullptr);
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(GN_THREADS), 0, st, (const float*)workspace, seg_chunk_begin, nseg,
                       fabsf(grad_scale), max_norm, seg_norm, norm_state, (const float*)nullptr);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}

extern "C" int ia_adamw_step_segmented_clipped(float* theta, const float* grad, float* exp_avg, float* exp_avg_sq,
                                               const int32_t* chunk_table, int nchunks, int32_t* seg_active, int32_t* seg_step,
                                               int nseg, int all_active, float lr, float beta1, float beta2, float eps,
                                               float weight_decay, float grad_scale, void* shadow_bf16, const float* norm_state,
                                               int skip_nonfinite, int32_t* counters, ia_stream_t stream) {
    const step_head h = make_head(theta, grad, exp_avg, exp_avg_sq, chunk_table, nchunks, seg_active, seg_step, nseg, all_active,
                                  beta1, beta2, eps, grad_scale, shadow_bf16, nullptr, norm_state, skip_nonfinite, counters);
    if (!norm_state || !counters || !head_ok(h)) return IA_INVALID_VALUE;
    return run_step(h, one_group(lr, weight_decay), plain_step{}, step_extras{}, (hipStream_t)stream);
}

extern "C" int ia_adamw_step_segmented_si(float* theta, const float* grad, float* exp_avg, float* exp_avg_sq,
                                          const int32_t* chunk_table, int nchunks, int32_t* seg_active, int32_t* seg_step, int nseg,
                                          int all_active, float lr, float beta1, float beta2, float eps, float weight_decay,
                                          float grad_scale, void* shadow_bf16, const float* norm_state, int skip_nonfinite,
                                          int32_t* counters, float* path_w, const float* omega, const float* theta_star,
                                          float penalty_coef, ia_stream_t stream) {
    const step_head h = make_head(theta, grad, exp_avg, exp_avg_sq, chunk_table, nchunks, seg_active, seg_step, nseg, all_active,
                                  beta1, beta2, eps, grad_scale, shadow_bf16, nullptr, norm_state, skip_nonfinite, counters);
    if (!head_ok(h) || !si_operands_ok(path_w, omega, theta_star)) return IA_INVALID_VALUE;
    return run_step_si(h, one_group(lr, weight_decay), path_w, omega, theta_star, penalty_coef, (hipStream_t)stream);
}

extern "C" int ia_si_consolidate(const float* theta, float* theta_star, float* path_w, float* omega, float xi, int64_t n,
                                 ia_stream_t stream) {
    if (!theta || !theta_star || !path_w || !omega || n <= 0 || !(xi > 0.f)) return IA_INVALID_VALUE;
    if (!ia_is_aligned(theta, 16) || !ia_is_aligned(theta_star, 16) || !ia_is_aligned(path_w, 16) || !ia_is_aligned(omega, 16))
        return IA_INVALID_VALUE;
    hipLaunchKernelGGL(si_consolidate_kernel, dim3(cap_grid(n >> 2, CL_THREADS * 4)), dim3(CL_THREADS), 0, (hipStream_t)stream,
                       theta, theta_star, path_w, omega, xi, n);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}

// The operands that are present select the variant: path_w, anchor and score together (scores) or none of them (EWC++ alone);
// importance and theta_star together (a language has been consolidated) or neither; a fold only with scores.
extern "C" int ia_adamw_step_segmented_rwalk(float* theta, const float* grad, float* exp_avg, float* exp_avg_sq,
                                             const int32_t* chunk_table, int nchunks, int32_t* seg_active, int32_t* seg_step,
                                             int nseg, int all_active, float beta1, float beta2, float eps, float grad_scale,
                                             void* shadow_bf16, const int32_t* seg_group, int ngroups, const float* group_lr,
                                             const float* group_weight_decay, const float* norm_state, int skip_nonfinite,
                                             int32_t* counters, float* fisher, float* path_w, float* anchor, float* score,
                                             const float* importance, const float* theta_star, float penalty_coef, float alpha,
                                             float fold_eps, int fold, ia_stream_t stream) {
    const step_head h = make_head(theta, grad, exp_avg, exp_avg_sq, chunk_table, nchunks, seg_active, seg_step, nseg, all_active,
                                  beta1, beta2, eps, grad_scale, shadow_bf16, seg_group, norm_state, skip_nonfinite, counters);
    const bool scores = path_w || anchor || score, pen = importance || theta_star;
    if (!head_ok(h) || !groups_ok(seg_group, ngroups, group_lr, group_weight_decay) ||
        !rwalk_operands_ok(fisher, path_w, anchor, score, importance, theta_star) || (fold && !scores) ||
        !(alpha > 0.f && alpha <= 1.f) || !(fold_eps > 0.f))
        return IA_INVALID_VALUE;
    const group_table gt = make_group_table(ngroups, group_lr, group_weight_decay);
    const float c2 = 2.f * penalty_coef;
    const auto run = [&](auto p, auto s, auto f) {
        return run_step(h, gt, rwalk_step<p(), s(), f()>{fisher, path_w, anchor, score, importance, theta_star, c2, alpha,
                                                         fold_eps}, step_extras{}, (hipStream_t)stream);
    };
    constexpr std::true_type yes;
    constexpr std::false_type no;
    if (pen) return !scores ? run(yes, no, no) : fold ? run(yes, yes, yes) : run(yes, yes, no);
    return !scores ? run(no, no, no) : fold ? run(no, yes, yes) : run(no, yes, no);
}

extern "C" size_t ia_rwalk_workspace_bytes(int nchunks) { return nchunks > 0 ? (size_t)nchunks * 2 * sizeof(float) : 0; }

extern "C" int ia_rwalk_consolidate(const float* theta, float* theta_star, const float* fisher, float* path_w, float* anchor,
                                    float* score, float* score_acc, float* importance, float* maxima, float fold_eps,
                                    int normalize, int first, int64_t n, const int32_t* chunk_table, int nchunks, void* workspace,
                                    size_t workspace_bytes, ia_stream_t stream) {
    const bool scores = path_w || anchor || score || score_acc;
    if (!theta || !theta_star || !fisher || !importance || !maxima || !chunk_table || !workspace || n <= 0 || nchunks <= 0 ||
        (scores && (!path_w || !anchor || !score || !score_acc)) || !(fold_eps > 0.f))
        return IA_INVALID_VALUE;
    if (!ia_is_aligned(theta, 16) || !ia_is_aligned(theta_star, 16) || !ia_is_aligned(fisher, 16) ||
        !ia_is_aligned(importance, 16) || !ia_is_aligned(maxima, 4) || !ia_is_aligned(chunk_table, 16) ||
        !ia_is_aligned(workspace, 8) ||
        (scores && (!ia_is_aligned(path_w, 16) || !ia_is_aligned(anchor, 16) || !ia_is_aligned(score, 16) ||
                    !ia_is_aligned(score_acc, 16))))
        return IA_INVALID_VALUE;
    if (workspace_bytes < ia_rwalk_workspace_bytes(nchunks)) return IA_WORKSPACE_TOO_SMALL;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(chunk_grid(nchunks)), flat_grid(cap_grid(n >> 2, CL_THREADS * 4)), block(CL_THREADS);
    const int4* table = (const int4*)chunk_table;
    float2* chunk_max = (float2*)workspace;
    if (scores)
        hipLaunchKernelGGL(rwalk_fold_max_kernel<true>, grid, block, 0, st, theta, fisher, path_w, anchor, score, fold_eps, table,
                           nchunks, chunk_max);
    else
        hipLaunchKernelGGL(rwalk_fold_max_kernel<false>, grid, block, 0, st, theta, fisher, path_w, anchor, score, fold_eps, table,
                           nchunks, chunk_max);
    hipLaunchKernelGGL(rwalk_max_finish_kernel, dim3(1), block, 0, st, (const float2*)chunk_max, nchunks, maxima);
    if (scores)
        hipLaunchKernelGGL(rwalk_combine_kernel<true>, flat_grid, block, 0, st, theta, theta_star, fisher, score, score_acc,
                           importance, (const float*)maxima, normalize, first, n);
    else
        hipLaunchKernelGGL(rwalk_combine_kernel<false>, flat_grid, block, 0, st, theta, theta_star, fisher, score, score_acc,
                           importance, (const float*)maxima, normalize, first, n);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}

extern "C" size_t ia_agem_workspace_bytes(int nchunks) { return nchunks > 0 ? (size_t)nchunks * 2 * sizeof(float) : 0; }

extern "C" int ia_agem_dots(const float* grad, const float* ref, const int32_t* chunk_table, int nchunks, int nseg,
                            float grad_scale, int32_t* seg_active, float* proj_state, void* workspace, size_t workspace_bytes,
                            ia_stream_t stream) {
    if (!grad || !ref || !chunk_table || !proj_state || !workspace || nchunks <= 0 || nseg <= 0) return IA_INVALID_VALUE;
    if (!ia_is_aligned(grad, 16) || !ia_is_aligned(ref, 16) || !ia_is_aligned(chunk_table, 16) || !ia_is_aligned(proj_state, 4) ||
        !ia_is_aligned(workspace, 8))
        return IA_INVALID_VALUE;
    if (workspace_bytes < ia_agem_workspace_bytes(nchunks)) return IA_WORKSPACE_TOO_SMALL;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(agem_dots_kernel, dim3(nchunks < 2048 ? nchunks : 2048), dim3(CL_THREADS), 0, st, grad, ref,
                       (const int4*)chunk_table, nchunks, seg_active, (float2*)workspace);
    hipLaunchKernelGGL(agem_finish_kernel, dim3(1), dim3(GN_THREADS), 0, st, (const float2*)workspace, nchunks, grad_scale,
                       proj_state);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}

extern "C" int ia_grad_norm_projected(const float* grad, const int32_t* chunk_table, int nchunks, const int32_t* seg_chunk_begin,
                                      int nseg, float grad_scale, float max_norm, const int32_t* seg_active, float* seg_norm,
                                      float* norm_state, void* workspace, size_t workspace_bytes, const float* ref,
                                      const float* proj_state, ia_stream_t stream) {
    if (!norm_operands_ok(grad, chunk_table, nchunks, seg_chunk_begin, nseg, seg_norm, norm_state, workspace) || !ref ||
        !proj_state || !ia_is_aligned(ref, 16) || !ia_is_aligned(proj_state, 4))
        return IA_INVALID_VALUE;
    if (workspace_bytes < ia_grad_norm_workspace_bytes(nchunks)) return IA_WORKSPACE_TOO_SMALL;
    return run_consumed_norm(grad, chunk_table, nchunks, seg_chunk_begin, nseg, grad_scale, max_norm, seg_active, seg_norm,
                             norm_state, workspace, agem_source{ref, proj_state}, proj_state + 3, (hipStream_t)stream);
}

extern "C" int ia_adamw_step_segmented_projected(float* theta, const float* grad, float* exp_avg, float* exp_avg_sq,
                                                 const int32_t* chunk_table, int nchunks, int32_t* seg_active, int32_t* seg_step,
                                                 int nseg, int all_active, float lr, float beta1, float beta2, float eps,
                                                 float weight_decay, float grad_scale, void* shadow_bf16, const float* norm_state,
                                                 int skip_nonfinite, int32_t* counters, const float* ref, const float* proj_state,
                                                 int32_t* proj_counters, ia_stream_t stream) {
    const step_head h = make_head(theta, grad, exp_avg, exp_avg_sq, chunk_table, nchunks, seg_active, seg_step, nseg, all_active,
                                  beta1, beta2, eps, grad_scale, shadow_bf16, nullptr, norm_state, skip_nonfinite, counters);
    if (!head_ok(h) || !proj_operands_ok(ref, proj_state, proj_counters)) return IA_INVALID_VALUE;
    return run_step_agem(h, one_group(lr, weight_decay), ref, proj_state, proj_counters, (hipStream_t)stream);
}

// The plain, clipped, SI or projected step with per-group lr / weight_decay: the operands that are present select the variant.
extern "C" int ia_adamw_step_segmented_grouped(float* theta, const float* grad, float* exp_avg, float* exp_avg_sq,
                                               const int32_t* chunk_table, int nchunks, int32_t* seg_active, int32_t* seg_step,
                                               int nseg, int all_active, float beta1, float beta2, float eps, float grad_scale,
                                               void* shadow_bf16, const int32_t* seg_group, int ngroups, const float* group_lr,
                                               const float* group_weight_decay, const float* norm_state, int skip_nonfinite,
                                               int32_t* counters, float* path_w, const float* omega, const float* theta_star,
                                               float penalty_coef, const float* ref, const float* proj_state,
                                               int32_t* proj_counters, ia_stream_t stream) {
    const step_head h = make_head(theta, grad, exp_avg, exp_avg_sq, chunk_table, nchunks, seg_active, seg_step, nseg, all_active,
                                  beta1, beta2, eps, grad_scale, shadow_bf16, seg_group, norm_state, skip_nonfinite, counters);
    const bool si = path_w || omega || theta_star, proj = ref || proj_state || proj_counters;
    if (!head_ok(h) || !groups_ok(seg_group, ngroups, group_lr, group_weight_decay) || (si && proj) ||
        (si && !si_operands_ok(path_w, omega, theta_star)) || (proj && !proj_operands_ok(ref, proj_state, proj_counters)))
        return IA_INVALID_VALUE;
    const group_table gt = make_group_table(ngroups, group_lr, group_weight_decay);
    hipStream_t st = (hipStream_t)stream;
    if (proj) return run_step_agem(h, gt, ref, proj_state, proj_counters, st);
    if (si) return run_step_si(h, gt, path_w, omega, theta_star, penalty_coef, st);
    return run_step(h, gt, plain_step{}, step_extras{}, st);
}

extern "C" size_t ia_gem_workspace_bytes(int nchunks, int max_tasks) {
    return nchunks > 0 && max_tasks >= 1 && max_tasks <= GEM_MAX ? (size_t)nchunks * max_tasks * sizeof(float) : 0;
}

extern "C" int ia_gem_dots(const float* x, const float* refs, int64_t stride, int ntasks, const int32_t* chunk_table, int nchunks,
                           int nseg, float grad_scale, int32_t* seg_active, int gram_row, double* gem_sums, void* workspace,
                           size_t workspace_bytes, ia_stream_t stream) {
    if (!x || !chunk_table || !workspace || !gem_sums || nchunks <= 0 || nseg <= 0 || gram_row >= ntasks || stride <= 0 ||
        (stride & 3) || !refs || ntasks < 1 || ntasks > GEM_MAX)
        return IA_INVALID_VALUE;
    if (!ia_is_aligned(refs, 16) || !ia_is_aligned(gem_sums, 8)) return IA_INVALID_VALUE;
    if (!ia_is_aligned(x, 16) || !ia_is_aligned(chunk_table, 16) || !ia_is_aligned(workspace, 4)) return IA_INVALID_VALUE;
    if (workspace_bytes < ia_gem_workspace_bytes(nchunks, ntasks)) return IA_WORKSPACE_TOO_SMALL;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(gem_dots_kernel, dim3(nchunks < 2048 ? nchunks : 2048), dim3(CL_THREADS), 0, st, x, refs, stride, ntasks,
                       (const int4*)chunk_table, nchunks, gram_row < 0 ? seg_active : (int32_t*)nullptr, (float*)workspace);
    hipLaunchKernelGGL(gem_finish_kernel, dim3(1), dim3(GN_THREADS), 0, st, (const float*)workspace, nchunks, ntasks, grad_scale,
                       gram_row, gem_sums);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}

extern "C" int ia_gem_solve(const double* gem_sums, float* gem_state, int ntasks, float memory_strength, float eps,
                            ia_stream_t stream) {
    if (!gem_state || !gem_sums || ntasks < 1 || ntasks > GEM_MAX || !(memory_strength >= 0.f) || !(eps >= 0.f) ||
        !isfinite(memory_strength) || !isfinite(eps))
        return IA_INVALID_VALUE;
    if (!ia_is_aligned(gem_state, 4) || !ia_is_aligned(gem_sums, 8)) return IA_INVALID_VALUE;
    hipLaunchKernelGGL(gem_solve_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, gem_sums, gem_state, ntasks, memory_strength,
                       eps);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}

extern "C" int ia_grad_norm_gem(const float* grad, const int32_t* chunk_table, int nchunks, const int32_t* seg_chunk_begin, int nseg,
                                float grad_scale, float max_norm, const int32_t* seg_active, float* seg_norm, float* norm_state,
                                void* workspace, size_t workspace_bytes, const float* refs, int64_t stride, int ntasks,
                                const float* gem_state, ia_stream_t stream) {
    if (!norm_operands_ok(grad, chunk_table, nchunks, seg_chunk_begin, nseg, seg_norm, norm_state, workspace) ||
        !gem_operands_ok(refs, stride, ntasks, gem_state))
        return IA_INVALID_VALUE;
    if (workspace_bytes < ia_grad_norm_workspace_bytes(nchunks)) return IA_WORKSPACE_TOO_SMALL;
    return run_consumed_norm(grad, chunk_table, nchunks, seg_chunk_begin, nseg, grad_scale, max_norm, seg_active, seg_norm,
                             norm_state, workspace, gem_source{refs, stride, ntasks, gem_state}, gem_state + GEM_VIOLATED,
                             (hipStream_t)stream);
}

extern "C" int ia_adamw_step_segmented_gem(float* theta, const float* grad, float* exp_avg, float* exp_avg_sq,
                                           const int32_t* chunk_table, int nchunks, int32_t* seg_active, int32_t* seg_step, int nseg,
                                           int all_active, float beta1, float beta2, float eps, float grad_scale, void* shadow_bf16,
                                           const int32_t* seg_group, int ngroups, const float* group_lr,
                                           const float* group_weight_decay, const float* norm_state, int skip_nonfinite,
                                           int32_t* counters, const float* refs, int64_t stride, int ntasks, const float* gem_state,
                                           int32_t* gem_counters, ia_stream_t stream) {
    const step_head h = make_head(theta, grad, exp_avg, exp_avg_sq, chunk_table, nchunks, seg_active, seg_step, nseg, all_active,
                                  beta1, beta2, eps, grad_scale, shadow_bf16, seg_group, norm_state, skip_nonfinite, counters);
    if (!head_ok(h) || !groups_ok(seg_group, ngroups, group_lr, group_weight_decay) || !gem_counters ||
        !ia_is_aligned(gem_counters, 4) || !gem_operands_ok(refs, stride, ntasks, gem_state))
        return IA_INVALID_VALUE;
    step_extras x = {};
    x.flags_preset = true;
    x.projected = gem_state + GEM_VIOLATED;
    x.projected_count = gem_counters;          // gem_counters = {projected steps, unsolved steps}
    x.solved = gem_state + GEM_SOLVED;
    x.unsolved_count = gem_counters + 1;
    return run_step(h, make_group_table(ngroups, group_lr, group_weight_decay), gem_step{{refs, stride, ntasks, gem_state}}, x,
                    (hipStream_t)stream);
}

extern "C" size_t ia_ogd_workspace_bytes(int nchunks, int max_rows) {
    return nchunks > 0 && max_rows >= 1 && max_rows <= IA_OGD_MAX_ROWS ? (size_t)nchunks * (max_rows + 1) * sizeof(float) : 0;
}

namespace {
inline bool ogd_operands_ok(const float* x, const float* basis, int64_t stride, int64_t numel, int nrows,
                            const int32_t* chunk_table, int nchunks, int nseg, const int32_t* seg_scope) {
    if (!x || !basis || !chunk_table || !seg_scope || nchunks <= 0 || nseg <= 0 || nrows < 1 || nrows > IA_OGD_MAX_ROWS ||
        numel <= 0 || stride < numel || (stride & 3))
        return false;
    return ia_is_aligned(x, 16) && ia_is_aligned(basis, 16) && ia_is_aligned(chunk_table, 16) && ia_is_aligned(seg_scope, 4);
}
}  // namespace

extern "C" int ia_ogd_dots(const float* x, const float* basis, int64_t stride, int64_t numel, int nrows,
                           const int32_t* chunk_table, int nchunks, int nseg, const int32_t* seg_scope, int32_t* seg_active,
                           int with_sq, double* dots64, float* dots32, void* workspace, size_t workspace_bytes,
                           ia_stream_t stream) {
    if (!ogd_operands_ok(x, basis, stride, numel, nrows, chunk_table, nchunks, nseg, seg_scope) || !dots64 || !dots32 ||
        !workspace)
        return IA_INVALID_VALUE;
    if (!ia_is_aligned(dots64, 8) || !ia_is_aligned(dots32, 4) || !ia_is_aligned(workspace, 4) ||
        (seg_active && !ia_is_aligned(seg_active, 4)))
        return IA_INVALID_VALUE;
    if (workspace_bytes < ia_ogd_workspace_bytes(nchunks, nrows)) return IA_WORKSPACE_TOO_SMALL;
    hipStream_t st = (hipStream_t)stream;
    auto kernel = with_sq ? ogd_dots_kernel<true> : ogd_dots_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(chunk_grid(nchunks)), dim3(CL_THREADS), 0, st, x, basis, stride, nrows,
                       (const int4*)chunk_table, nchunks, seg_scope, seg_active, (float*)workspace);
    hipLaunchKernelGGL(ogd_finish_kernel, dim3(nrows + (with_sq ? 1 : 0)), dim3(GN_THREADS), 0, st, (const float*)workspace,
                       nchunks, dots64, dots32);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}

extern "C" int ia_ogd_project(const float* x, const float* basis, int64_t stride, int64_t numel, int nrows, const float* coef,
                              float alpha, const int32_t* chunk_table, int nchunks, int nseg, const int32_t* seg_scope,
                              const int32_t* seg_active, float* dst, ia_stream_t stream) {
    if (!ogd_operands_ok(x, basis, stride, numel, nrows, chunk_table, nchunks, nseg, seg_scope) || !coef || !dst)
        return IA_INVALID_VALUE;
    if (!ia_is_aligned(coef, 4) || !ia_is_aligned(dst, 16) || (seg_active && !ia_is_aligned(seg_active, 4)))
        return IA_INVALID_VALUE;
    hipLaunchKernelGGL(ogd_project_kernel, dim3(chunk_grid(nchunks)), dim3(CL_THREADS), 0, (hipStream_t)stream, x, basis, stride,
                       nrows, coef, alpha, (const int4*)chunk_table, nchunks, seg_scope, seg_active, dst);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}

extern "C" int ia_adamw_step_segmented_masked(float* theta, const float* grad, float* exp_avg, float* exp_avg_sq,
                                              const int32_t* chunk_table, int nchunks, int32_t* seg_active, int32_t* seg_step,
                                              int nseg, int all_active, float beta1, float beta2, float eps, float grad_scale,
                                              void* shadow_bf16, const int32_t* seg_group, int ngroups, const float* group_lr,
                                              const float* group_weight_decay, const float* norm_state, int skip_nonfinite,
                                              int32_t* counters, const float* base, float* scores, const int32_t* seg_kind,
                                              float threshold, ia_stream_t stream) {
    const step_head h = make_head(theta, grad, exp_avg, exp_avg_sq, chunk_table, nchunks, seg_active, seg_step, nseg, all_active,
                                  beta1, beta2, eps, grad_scale, shadow_bf16, seg_group, norm_state, skip_nonfinite, counters);
    if (!head_ok(h) || !groups_ok(seg_group, ngroups, group_lr, group_weight_decay) || !base || !scores || !seg_kind ||
        !ia_is_aligned(base, 16) || !ia_is_aligned(scores, 16) || !ia_is_aligned(seg_kind, 4))
        return IA_INVALID_VALUE;
    step_extras x = {};
    x.seg_kind = seg_kind;
    return run_step(h, make_group_table(ngroups, group_lr, group_weight_decay), masked_step{base, scores, seg_kind, threshold}, x,
                    (hipStream_t)stream);
}

// The plain grouped step with two things left to the caller: which tensors it may touch (seg_kind, NULL: all of them) and, with
// flags_preset, the liveness flags themselves.  The walker, the update rule and the advance are those of every other step.
extern "C" int ia_adamw_step_segmented_kinds(float* theta, const float* grad, float* exp_avg, float* exp_avg_sq,
                                             const int32_t* chunk_table, int nchunks, int32_t* seg_active, int32_t* seg_step,
                                             int nseg, int all_active, float beta1, float beta2, float eps, float grad_scale,
                                             void* shadow_bf16, const int32_t* seg_group, int ngroups, const float* group_lr,
                                             const float* group_weight_decay, const float* norm_state, int skip_nonfinite,
                                             int32_t* counters, const int32_t* seg_kind, int flags_preset, ia_stream_t stream) {
    const step_head h = make_head(theta, grad, exp_avg, exp_avg_sq, chunk_table, nchunks, seg_active, seg_step, nseg, all_active,
                                  beta1, beta2, eps, grad_scale, shadow_bf16, seg_group, norm_state, skip_nonfinite, counters);
    if (!head_ok(h) || !groups_ok(seg_group, ngroups, group_lr, group_weight_decay) || (seg_kind && !ia_is_aligned(seg_kind, 4)) ||
        (flags_preset && all_active))
        return IA_INVALID_VALUE;
    step_extras x = {};
    x.flags_preset = flags_preset != 0;
    x.seg_kind = seg_kind;
    x.free_only = seg_kind != nullptr;
    const group_table gt = make_group_table(ngroups, group_lr, group_weight_decay);
    return seg_kind ? run_step(h, gt, kinds_step{seg_kind}, x, (hipStream_t)stream)
                    : run_step(h, gt, plain_step{}, x, (hipStream_t)stream);
}

extern "C" int ia_mask_pack(const float* scores, const int32_t* chunk_table, int nchunks, const int32_t* seg_kind, int nseg,
                            float threshold, uint64_t* bits, int64_t nwords, int32_t* seg_kept, ia_stream_t stream) {
    if (!scores || !chunk_table || !seg_kind || !bits || nchunks <= 0 || nseg <= 0 || nwords <= 0) return IA_INVALID_VALUE;
    if (!ia_is_aligned(scores, 16) || !ia_is_aligned(chunk_table, 16) || !ia_is_aligned(seg_kind, 4) || !ia_is_aligned(bits, 8) ||
        (seg_kept && !ia_is_aligned(seg_kept, 4)))
        return IA_INVALID_VALUE;
    hipStream_t st = (hipStream_t)stream;
    if (seg_kept && hipMemsetAsync(seg_kept, 0, (size_t)nseg * sizeof(int32_t), st) != hipSuccess) return IA_LAUNCH_FAILED;
    hipLaunchKernelGGL(mask_pack_kernel, dim3(nchunks < 2048 ? nchunks : 2048), dim3(CL_THREADS), 0, st, scores,
                       (const int4*)chunk_table, nchunks, seg_kind, threshold, (unsigned long long*)bits, nwords, seg_kept);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}

extern "C" int ia_mask_apply(float* theta, const float* base, const uint64_t* bits, int64_t nwords, const int32_t* chunk_table,
                             int nchunks, const int32_t* seg_kind, int nseg, void* shadow_bf16, ia_stream_t stream) {
    if (!theta || !base || !bits || !chunk_table || !seg_kind || nchunks <= 0 || nseg <= 0 || nwords <= 0) return IA_INVALID_VALUE;
    if (!ia_is_aligned(theta, 16) || !ia_is_aligned(base, 16) || !ia_is_aligned(bits, 8) || !ia_is_aligned(chunk_table, 16) ||
        !ia_is_aligned(seg_kind, 4) || (shadow_bf16 && !ia_is_aligned(shadow_bf16, 8)))
        return IA_INVALID_VALUE;
    hipLaunchKernelGGL(mask_apply_kernel, dim3(nchunks < 2048 ? nchunks : 2048), dim3(CL_THREADS), 0, (hipStream_t)stream, theta,
                       base, (const unsigned long long*)bits, nwords, (const int4*)chunk_table, nchunks, seg_kind,
                       (unsigned short*)shadow_bf16);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}

extern "C" int ia_grad_norm_packed(const float* grad, const int32_t* chunk_table, int nchunks, const int32_t* seg_chunk_begin,
                                   int nseg, float grad_scale, float max_norm, int32_t* seg_active, float* seg_norm,
                                   float* norm_state, void* workspace, size_t workspace_bytes, const uint8_t* owner,
                                   const int32_t* seg_kind, int train_owner, ia_stream_t stream) {
    if (!norm_operands_ok(grad, chunk_table, nchunks, seg_chunk_begin, nseg, seg_norm, norm_state, workspace) || !owner ||
        !seg_kind || !ia_is_aligned(owner, 16) || !ia_is_aligned(seg_kind, 4))
        return IA_INVALID_VALUE;
    if (workspace_bytes < ia_grad_norm_workspace_bytes(nchunks)) return IA_WORKSPACE_TOO_SMALL;
    hipStream_t st = (hipStream_t)stream;
    if (seg_active)      // liveness is the raw gradient's, as in ia_grad_norm's first pass
        hipLaunchKernelGGL(seg_activity_kernel<false>, dim3(chunk_grid(nchunks)), dim3(CL_THREADS), 0, st, grad,
                           (const int4*)chunk_table, nchunks, seg_active, (float*)nullptr, (const int32_t*)nullptr);
    return run_consumed_norm(grad, chunk_table, nchunks, seg_chunk_begin, nseg, grad_scale, max_norm, seg_active, seg_norm,
                             norm_state, workspace, packed_source{owner, seg_kind, train_owner}, (const float*)nullptr, st);
}

extern "C" int ia_adamw_step_segmented_packed(float* theta, const float* grad, float* exp_avg, float* exp_avg_sq,
                                              const int32_t* chunk_table, int nchunks, int32_t* seg_active, int32_t* seg_step,
                                              int nseg, int all_active, float beta1, float beta2, float eps, float grad_scale,
                                              void* shadow_bf16, const int32_t* seg_group, int ngroups, const float* group_lr,
                                              const float* group_weight_decay, const float* norm_state, int skip_nonfinite,
                                              int32_t* counters, const uint8_t* owner, const int32_t* seg_kind, int train_owner,
                                              ia_stream_t stream) {
    const step_head h = make_head(theta, grad, exp_avg, exp_avg_sq, chunk_table, nchunks, seg_active, seg_step, nseg, all_active,
                                  beta1, beta2, eps, grad_scale, shadow_bf16, seg_group, norm_state, skip_nonfinite, counters);
    if (!head_ok(h) || !groups_ok(seg_group, ngroups, group_lr, group_weight_decay) || !owner || !seg_kind ||
        !ia_is_aligned(owner, 16) || !ia_is_aligned(seg_kind, 4))
        return IA_INVALID_VALUE;
    step_extras x = {};
    x.seg_kind = seg_kind;
    return run_step(h, make_group_table(ngroups, group_lr, group_weight_decay), packed_step{owner, seg_kind, train_owner}, x,
                    (hipStream_t)stream);
}

// workspace: pack_sel[nseg], then the histograms unsigned[nseg][PK_BINS]
extern "C" size_t ia_pack_prune_workspace_bytes(int nseg) {
    return nseg > 0 ? (size_t)nseg * (sizeof(pack_sel) + PK_BINS * sizeof(unsigned)) : 0;
}

extern "C" int ia_pack_prune(float* theta, float* exp_avg, float* exp_avg_sq, uint8_t* owner, const int32_t* chunk_table,
                             int nchunks, const int32_t* seg_kind, int nseg, float fraction, int task, void* shadow_bf16,
                             int32_t* seg_counts, void* workspace, size_t workspace_bytes, ia_stream_t stream) {
    if (!theta || !exp_avg || !exp_avg_sq || !owner || !chunk_table || !seg_kind || !seg_counts || !workspace || nchunks <= 0 ||
        nseg <= 0 || task < 1 || task > 255 || !(fraction >= 0.f && fraction < 1.f))
        return IA_INVALID_VALUE;
    if (!ia_is_aligned(theta, 16) || !ia_is_aligned(exp_avg, 16) || !ia_is_aligned(exp_avg_sq, 16) || !ia_is_aligned(owner, 16) ||
        !ia_is_aligned(chunk_table, 16) || !ia_is_aligned(seg_kind, 4) || !ia_is_aligned(seg_counts, 4) ||
        !ia_is_aligned(workspace, 16) || (shadow_bf16 && !ia_is_aligned(shadow_bf16, 8)))
        return IA_INVALID_VALUE;
    const size_t need = ia_pack_prune_workspace_bytes(nseg);
    if (workspace_bytes < need) return IA_WORKSPACE_TOO_SMALL;
    hipStream_t st = (hipStream_t)stream;
    pack_sel* sel = (pack_sel*)workspace;
    unsigned* hist = (unsigned*)(sel + nseg);
    if (hipMemsetAsync(workspace, 0, need, st) != hipSuccess ||
        hipMemsetAsync(seg_counts, 0, (size_t)nseg * 2 * sizeof(int32_t), st) != hipSuccess)
        return IA_LAUNCH_FAILED;
    for (int pass = 0; pass < PK_PASSES; ++pass) {
        hipLaunchKernelGGL(pack_hist_kernel, dim3(chunk_grid(nchunks)), dim3(CL_THREADS), 0, st, theta, owner,
                           (const int4*)chunk_table, nchunks, seg_kind, sel, pass, hist);
        hipLaunchKernelGGL(pack_pick_kernel, dim3(nseg), dim3(PK_BINS), 0, st, hist, sel, seg_kind, pass, fraction,
                           seg_counts);
    }
    hipLaunchKernelGGL(pack_prune_kernel, dim3(chunk_grid(nchunks)), dim3(CL_THREADS), 0, st, theta, exp_avg, exp_avg_sq, owner,
                       (const int4*)chunk_table, nchunks, seg_kind, sel, task, (unsigned short*)shadow_bf16);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}

extern "C" int ia_pack_apply(float* theta, const float* base, const uint8_t* owner, const int32_t* chunk_table, int nchunks,
                             const int32_t* seg_kind, int nseg, int lo, int hi, void* shadow_bf16, ia_stream_t stream) {
    if (!theta || !base || !owner || !chunk_table || !seg_kind || nchunks <= 0 || nseg <= 0) return IA_INVALID_VALUE;
    if (!ia_is_aligned(theta, 16) || !ia_is_aligned(base, 16) || !ia_is_aligned(owner, 16) || !ia_is_aligned(chunk_table, 16) ||
        !ia_is_aligned(seg_kind, 4) || (shadow_bf16 && !ia_is_aligned(shadow_bf16, 8)))
        return IA_INVALID_VALUE;
    hipLaunchKernelGGL(pack_apply_kernel, dim3(chunk_grid(nchunks)), dim3(CL_THREADS), 0, (hipStream_t)stream, theta, base, owner,
                       (const int4*)chunk_table, nchunks, seg_kind, lo, hi, (unsigned short*)shadow_bf16);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}
