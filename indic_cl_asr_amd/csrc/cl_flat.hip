// Continual-learning regulariser + optimizer kernels over ONE flat fp32 buffer of all trainable parameters
// (the reference launches one set of elementwise kernels per tensor, ~300 per step: SURVEY.md §8 a17/a18/a20).
//   ia_cl_penalty ............ R/cl_baseline_ewc.py:69-81 (2*lambda*F*(theta-theta*), mean_k mean|.| monitor) and
//                              R/cl_baseline_mas.py:70-75 (sum omega*(theta-theta*)^2 and its gradient)
//   ia_cl_fisher_accumulate .. R/cl_baseline_ewc.py:245-255  F += mean(loss) * g^2
//   ia_cl_abs_accumulate ..... R/cl_baseline_mas.py:267-270  omega += |g|
//   ia_adamw_step ............ torch.optim.AdamW single-tensor update (R/cl_baseline.py:137 defaults)
//   ia_grad_norm ............. torch.nn.utils.clip_grad_norm_'s norm and coefficient of the flat gradient, on the device
//   ia_adamw_step_segmented_clipped .. the per-tensor AdamW on (g * grad_scale) * coef, skipped when the norm is not finite
//   ia_adamw_step_segmented_si ....... the same step with Synaptic Intelligence's path integral w -= ge * (theta' - theta) and,
//                              from the second task on, the surrogate's gradient 2c*omega*(theta-theta*) added after the clip
//   ia_si_consolidate ........ end of a task: omega += max(0, w / ((theta-theta*)^2 + xi)), w = 0, theta* = theta
//   ia_agem_dots ............. Averaged GEM (Chaudhry et al. 2019): g.r and r.r of the flat gradient and the episodic-memory
//                              reference gradient, the decision g.r < 0 and alpha = g.r / r.r left on the device
//   ia_grad_norm_projected ... ia_grad_norm of the gradient the projected step consumes (g - alpha * r when the flag is set)
//   ia_adamw_step_segmented_projected .. the per-tensor AdamW on that gradient, r as one more operand of the launch
//   ia_gem_dots, ia_gem_solve, ia_grad_norm_gem, ia_adamw_step_segmented_gem .. GEM (Lopez-Paz, Ranzato 2017): the K dots of the
//                              flat gradient with one reference row per earlier task (and the rows' Gram matrix), the
//                              bound-constrained quadratic program in fp64, and norm and AdamW on g * s + sum_k v_k * r_k
//   ia_adamw_step_segmented_grouped .... any of the four segmented steps with lr and weight_decay per parameter group
//                              (torch.optim.AdamW's param_groups): the same kernels, the group table by value in their arguments
//   ia_adamw_step_segmented_masked, ia_mask_pack, ia_mask_apply .. Piggyback (Mallya, Davis, Lazebnik 2018): per tensor a kind --
//                              masked (scores trained on g * base, theta = score >= threshold ? base : 0), free (the plain step),
//                              frozen (untouched) --, the scores as one bit per weight, and the bits back to weights
// All are HBM-streaming kernels: 16-byte accesses, grid capped at 2048 workgroups, fp32 math.
#include "ia_common.h"

namespace {
constexpr int CL_THREADS = 256;
constexpr int CL_CHUNK = 4096;  // elements per chunk-table entry (host builds the table with this size)

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
        if (shadow_bf16) {
            __hip_bfloat16 a = __float2bfloat16(P.x), b = __float2bfloat16(P.y), c = __float2bfloat16(P.z),
                           d = __float2bfloat16(P.w);
            ushort4 o;
            o.x = *reinterpret_cast<unsigned short*>(&a); o.y = *reinterpret_cast<unsigned short*>(&b);
            o.z = *reinterpret_cast<unsigned short*>(&c); o.w = *reinterpret_cast<unsigned short*>(&d);
            reinterpret_cast<ushort4*>(shadow_bf16)[q] = o;
        }
    }
    if (blockIdx.x == 0)
        for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += CL_THREADS) {
            float P = p[i], M = m[i], V = v[i];
            adamw1(P, g[i] * grad_scale, M, V, lr, b1, b2, eps, wd, step_size, inv_bc2_sqrt);
            p[i] = P; m[i] = M; v[i] = V;
            if (shadow_bf16) { __hip_bfloat16 a = __float2bfloat16(P); shadow_bf16[i] = *reinterpret_cast<unsigned short*>(&a); }
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
                                                                  float* __restrict__ chunk_sumsq) {
    __shared__ float sh[CL_THREADS / 64];
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int4 e = table[c];
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
// norm_state = {total_norm, coef, non-finite flag (0 / 1), max_norm}.
constexpr int GN_THREADS = 1024;
__device__ __forceinline__ void grad_norm_finish(const float* __restrict__ chunk_sumsq, const int* __restrict__ seg_chunk_begin,
                                                 int nseg, float abs_scale, float max_norm, float* __restrict__ seg_norm,
                                                 float* __restrict__ norm_state) {
    __shared__ double sh_w[GN_THREADS / 64];
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

__global__ __launch_bounds__(GN_THREADS) void grad_norm_finish_kernel(const float* __restrict__ chunk_sumsq,
                                                                      const int* __restrict__ seg_chunk_begin, int nseg,
                                                                      float abs_scale, float max_norm,
                                                                      float* __restrict__ seg_norm, float* __restrict__ norm_state) {
    grad_norm_finish(chunk_sumsq, seg_chunk_begin, nseg, abs_scale, max_norm, seg_norm, norm_state);
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

// CLIP: the gradient is (g * grad_scale) * coef with coef = norm_state[1] read from the device, each product rounded to
// fp32 on its own (never fused into the moment update), so that with grad_scale == 1 it is torch's g.mul_(coef) bit for
// bit; when norm_state[2] flags a non-finite norm and skip_nonfinite is set the launch writes nothing at all.
template <bool CLIP>
__device__ __forceinline__ float eff_grad(float g, float grad_scale, float coef) {
    if constexpr (!CLIP) {
        return g * grad_scale;
    } else {
#pragma clang fp contract(off)
        const float gs = g * grad_scale;
        return gs * coef;
    }
}

template <bool CLIP>
__global__ __launch_bounds__(CL_THREADS) void adamw_seg_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                               float* __restrict__ m, float* __restrict__ v,
                                                               const int4* __restrict__ table, int nchunks,
                                                               const int* __restrict__ seg_active,
                                                               const int* __restrict__ seg_step, const group_table groups,
                                                               const int* __restrict__ seg_group, float b1, float b2, float eps,
                                                               float grad_scale,
                                                               unsigned short* __restrict__ shadow_bf16,
                                                               const float* __restrict__ norm_state, int skip_nonfinite) {
    __shared__ float sh_c[2];
    float coef = 1.f;
    if (CLIP) {
        if (skip_nonfinite && norm_state[2] != 0.f) return;
        coef = norm_state[1];
    }
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int4 e = table[c];
        if (!seg_active[e.z]) {           // workgroup-uniform: untouched tensor -- only keep its bf16 image in step
            if (shadow_bf16)
                for (int i = threadIdx.x; i < e.y; i += CL_THREADS) {
                    __hip_bfloat16 a = __float2bfloat16(p[e.x + i]);
                    shadow_bf16[e.x + i] = *reinterpret_cast<unsigned short*>(&a);
                }
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
        const float step_size = sh_c[0], inv_bc2_sqrt = sh_c[1];
        const int off = e.x, cnt = e.y, n4 = cnt >> 2;
        for (int q = threadIdx.x; q < n4; q += CL_THREADS) {
            float4 P = reinterpret_cast<float4*>(p + off)[q];
            const float4 G = reinterpret_cast<const float4*>(g + off)[q];
            float4 M = reinterpret_cast<float4*>(m + off)[q];
            float4 V = reinterpret_cast<float4*>(v + off)[q];
            adamw1(P.x, eff_grad<CLIP>(G.x, grad_scale, coef), M.x, V.x, lr, b1, b2, eps, wd, step_size, inv_bc2_sqrt);
            adamw1(P.y, eff_grad<CLIP>(G.y, grad_scale, coef), M.y, V.y, lr, b1, b2, eps, wd, step_size, inv_bc2_sqrt);
            adamw1(P.z, eff_grad<CLIP>(G.z, grad_scale, coef), M.z, V.z, lr, b1, b2, eps, wd, step_size, inv_bc2_sqrt);
            adamw1(P.w, eff_grad<CLIP>(G.w, grad_scale, coef), M.w, V.w, lr, b1, b2, eps, wd, step_size, inv_bc2_sqrt);
            reinterpret_cast<float4*>(p + off)[q] = P;
            reinterpret_cast<float4*>(m + off)[q] = M;
            reinterpret_cast<float4*>(v + off)[q] = V;
            if (shadow_bf16) {
                __hip_bfloat16 a = __float2bfloat16(P.x), b = __float2bfloat16(P.y), cc = __float2bfloat16(P.z),
                               d = __float2bfloat16(P.w);
                ushort4 o;
                o.x = *reinterpret_cast<unsigned short*>(&a); o.y = *reinterpret_cast<unsigned short*>(&b);
                o.z = *reinterpret_cast<unsigned short*>(&cc); o.w = *reinterpret_cast<unsigned short*>(&d);
                reinterpret_cast<ushort4*>(shadow_bf16 + off)[q] = o;
            }
        }
        for (int i = (n4 << 2) + threadIdx.x; i < cnt; i += CL_THREADS) {
            float P = p[off + i], M = m[off + i], V = v[off + i];
            adamw1(P, eff_grad<CLIP>(g[off + i], grad_scale, coef), M, V, lr, b1, b2, eps, wd, step_size, inv_bc2_sqrt);
            p[off + i] = P; m[off + i] = M; v[off + i] = V;
            if (shadow_bf16) { __hip_bfloat16 a = __float2bfloat16(P); shadow_bf16[off + i] = *reinterpret_cast<unsigned short*>(&a); }
        }
    }
}

// ---- Synaptic Intelligence (Zenke, Poole, Ganguli 2017) inside the AdamW launch.  Per element of a live tensor:
//   ge = g * grad_scale                      the task gradient (before the clip coefficient, without the penalty)
//   G  = ge [* coef] [+ (c2 * omega) * (theta - theta_star)]      the gradient AdamW consumes (PEN: a penalty is attached)
//   theta', m, v = adamw1(theta, G, ...)
//   w  = w - ge * (theta' - theta)           the path integral, on the fp32 weight that is stored (weight decay included)
// Every product, difference and sum of these lines is rounded to fp32 on its own (contraction off), so that one torch op
// per rounding reproduces G and w bit for bit; adamw1 itself is the routine of the plain kernel.
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

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

// adamw1 with every rounding written out.  Left to the compiler, the contraction of adamw1 depends on the code around it: in
// adamw_seg_kernel (both instantiations) it comes out as below, the second moment as fma(g, (1-b2)*g, b2*v) in the float4 body
// and as fma(b2, v, ((1-b2)*g)*g) in the scalar tail; inside this kernel the same source lost some of the fmas.  The SI step has
// to move the weights exactly as the plain step does on the same gradient (an element is in the body of both kernels or in the
// tail of both), so it restates that arithmetic with explicit fmas; tests/test_si_gpu.py compares the two bit for bit.
template <bool TAIL>
__device__ __forceinline__ void adamw1_rn(float& p, float g, float& m, float& v, float decay, float omb1, float b2, float omb2,
                                          float eps, float step_size, float inv_bc2_sqrt) {
#pragma clang fp contract(off)
    const float t = omb2 * g;
    if constexpr (TAIL) {
        const float tg = t * g;
        v = __builtin_fmaf(b2, v, tg);
    } else {
        const float vb = b2 * v;
        v = __builtin_fmaf(g, t, vb);
    }
    const float gm = g - m;
    m = __builtin_fmaf(omb1, gm, m);
    const float denom = __builtin_fmaf(inv_bc2_sqrt, sqrtf(v), eps);
    const float q = m / denom;
    const float u = step_size * q;
    p = __builtin_fmaf(decay, p, -u);
}

struct si_consts {   // workgroup-uniform operands of one chunk
    float decay, omb1, b2, omb2, eps, step_size, inv_bc2_sqrt, grad_scale, coef, c2;
};

template <bool CLIP, bool PEN, bool TAIL>
__device__ __forceinline__ void adamw_si1(float& p, float g, float& m, float& v, float& w, float omega, float star,
                                          const si_consts& k) {
    const float ge = mul_rn(g, k.grad_scale);
    const float eff = CLIP ? mul_rn(ge, k.coef) : ge;           // eff_grad<true>'s two products
    const float p_old = p;
    adamw1_rn<TAIL>(p, si_grad<PEN>(eff, p_old, omega, star, k.c2), m, v, k.decay, k.omb1, k.b2, k.omb2, k.eps, k.step_size,
                    k.inv_bc2_sqrt);
    w = si_path(w, ge, p, p_old);
}

template <bool CLIP, bool PEN>
__global__ __launch_bounds__(CL_THREADS) void adamw_seg_si_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                  float* __restrict__ m, float* __restrict__ v,
                                                                  const int4* __restrict__ table, int nchunks,
                                                                  const int* __restrict__ seg_active,
                                                                  const int* __restrict__ seg_step, const group_table groups,
                                                                  const int* __restrict__ seg_group, float b1, float b2, float eps,
                                                                  float grad_scale,
                                                                  unsigned short* __restrict__ shadow_bf16,
                                                                  const float* __restrict__ norm_state, int skip_nonfinite,
                                                                  float* __restrict__ path_w, const float* __restrict__ omega,
                                                                  const float* __restrict__ star, float c2) {
    __shared__ float sh_c[2];
    float coef = 1.f;
    if (CLIP) {
        if (skip_nonfinite && norm_state[2] != 0.f) return;
        coef = norm_state[1];
    }
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int4 e = table[c];
        if (!seg_active[e.z]) {           // workgroup-uniform: untouched tensor -- its w stays, only the bf16 image is kept in step
            if (shadow_bf16)
                for (int i = threadIdx.x; i < e.y; i += CL_THREADS) {
                    __hip_bfloat16 a = __float2bfloat16(p[e.x + i]);
                    shadow_bf16[e.x + i] = *reinterpret_cast<unsigned short*>(&a);
                }
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
        const si_consts k = {__builtin_fmaf(-lr, wd, 1.f), 1.f - b1, b2, 1.f - b2, eps, sh_c[0], sh_c[1], grad_scale, coef, c2};
        const int off = e.x, cnt = e.y, n4 = cnt >> 2;
        for (int q = threadIdx.x; q < n4; q += CL_THREADS) {
            float4 P = reinterpret_cast<float4*>(p + off)[q];
            const float4 G = reinterpret_cast<const float4*>(g + off)[q];
            float4 M = reinterpret_cast<float4*>(m + off)[q];
            float4 V = reinterpret_cast<float4*>(v + off)[q];
            float4 W = reinterpret_cast<float4*>(path_w + off)[q];
            float4 O = make_float4(0.f, 0.f, 0.f, 0.f), S = O;
            if constexpr (PEN) {
                O = reinterpret_cast<const float4*>(omega + off)[q];
                S = reinterpret_cast<const float4*>(star + off)[q];
            }
            adamw_si1<CLIP, PEN, false>(P.x, G.x, M.x, V.x, W.x, O.x, S.x, k);
            adamw_si1<CLIP, PEN, false>(P.y, G.y, M.y, V.y, W.y, O.y, S.y, k);
            adamw_si1<CLIP, PEN, false>(P.z, G.z, M.z, V.z, W.z, O.z, S.z, k);
            adamw_si1<CLIP, PEN, false>(P.w, G.w, M.w, V.w, W.w, O.w, S.w, k);
            reinterpret_cast<float4*>(p + off)[q] = P;
            reinterpret_cast<float4*>(m + off)[q] = M;
            reinterpret_cast<float4*>(v + off)[q] = V;
            reinterpret_cast<float4*>(path_w + off)[q] = W;
            if (shadow_bf16) {
                __hip_bfloat16 a = __float2bfloat16(P.x), b = __float2bfloat16(P.y), cc = __float2bfloat16(P.z),
                               d = __float2bfloat16(P.w);
                ushort4 o;
                o.x = *reinterpret_cast<unsigned short*>(&a); o.y = *reinterpret_cast<unsigned short*>(&b);
                o.z = *reinterpret_cast<unsigned short*>(&cc); o.w = *reinterpret_cast<unsigned short*>(&d);
                reinterpret_cast<ushort4*>(shadow_bf16 + off)[q] = o;
            }
        }
        for (int i = (n4 << 2) + threadIdx.x; i < cnt; i += CL_THREADS) {
            float P = p[off + i], M = m[off + i], V = v[off + i], W = path_w[off + i];
            const float O = PEN ? omega[off + i] : 0.f, S = PEN ? star[off + i] : 0.f;
            adamw_si1<CLIP, PEN, true>(P, g[off + i], M, V, W, O, S, k);
            p[off + i] = P; m[off + i] = M; v[off + i] = V; path_w[off + i] = W;
            if (shadow_bf16) { __hip_bfloat16 a = __float2bfloat16(P); shadow_bf16[off + i] = *reinterpret_cast<unsigned short*>(&a); }
        }
    }
}

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

// ---- Averaged GEM (Chaudhry, Ranzato, Rohrbach, Elhoseiny 2019).  r is the gradient of a batch drawn from the episodic memory,
// stored averaged and in true units; g is the flat task gradient, still to be multiplied by grad_scale.  When g.r < 0 the step
// consumes g - (g.r / r.r) * r.  Three passes, none with a float atomic, each with a fixed summation order:
//   agem_dots_kernel     workgroup c leaves {sum g*r, sum r*r} of chunk c (fp32, the reduction shape of
//                        seg_activity_kernel<true>) in chunk_dots[c] and sets the liveness flags from g as that kernel does
//   agem_finish_kernel   one workgroup adds the partials in fp64 (thread t takes chunks t, t + 1024, ...; butterfly over the
//                        lanes; thread 0 adds the 16 wave totals in order) and writes proj_state = {dot, ref_sq, alpha, violated}
//   proj_norm_kernel     the chunk sums of squares of the gradient the step will consume, branching on the device flag
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

__device__ __forceinline__ float sub_rn(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}

// (g * grad_scale) - (alpha * r): both products and the difference rounded to fp32 on their own
__device__ __forceinline__ float proj_grad(float g, float r, float grad_scale, float alpha) {
    return sub_rn(mul_rn(g, grad_scale), mul_rn(alpha, r));
}

// seg_activity_kernel<true>'s sum as the compiler emits it there, written out so that an un-projected step measures the norm
// ia_grad_norm measures bit for bit (tests/test_agem_gpu.py compares them): in the float4 body four separately rounded squares
// added left to right and then to the running sum, in the scalar tail one fma.
__device__ __forceinline__ float sumsq4_rn(float ss, float a, float b, float c, float d) {
#pragma clang fp contract(off)
    const float aa = a * a, bb = b * b, cc = c * c, dd = d * d;
    const float t = ((aa + bb) + cc) + dd;
    return ss + t;
}

// violated == 0: the raw sum of g^2 over every chunk, as ia_grad_norm's first pass.  violated == 1: the sum of G^2 with
// G = g * grad_scale - alpha * r over the chunks of live tensors; a dead tensor's chunk stores 0 (its .grad is None for torch's
// clip norm) and is not read.  seg_active is read only (NULL: every tensor live): agem_dots_kernel has set it.
__global__ __launch_bounds__(CL_THREADS) void proj_norm_kernel(const float* __restrict__ g, const float* __restrict__ r,
                                                               const int4* __restrict__ table, int nchunks,
                                                               const int* __restrict__ seg_active,
                                                               const float* __restrict__ proj_state, float grad_scale,
                                                               float* __restrict__ chunk_sumsq) {
    __shared__ float sh[CL_THREADS / 64];
    const bool violated = proj_state[3] != 0.f;
    const float alpha = proj_state[2];
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int4 e = table[c];
        const int off = e.x, cnt = e.y, n4 = cnt >> 2;
        float ss = 0.f;
        if (!violated) {
            for (int q = threadIdx.x; q < n4; q += CL_THREADS) {
                const float4 x = reinterpret_cast<const float4*>(g + off)[q];
                ss = sumsq4_rn(ss, x.x, x.y, x.z, x.w);
            }
            for (int i = (n4 << 2) + threadIdx.x; i < cnt; i += CL_THREADS) ss = __builtin_fmaf(g[off + i], g[off + i], ss);
        } else if (!seg_active || seg_active[e.z]) {
            for (int q = threadIdx.x; q < n4; q += CL_THREADS) {
                const float4 x = reinterpret_cast<const float4*>(g + off)[q];
                const float4 y = reinterpret_cast<const float4*>(r + off)[q];
                ss = sumsq4_rn(ss, proj_grad(x.x, y.x, grad_scale, alpha), proj_grad(x.y, y.y, grad_scale, alpha),
                               proj_grad(x.z, y.z, grad_scale, alpha), proj_grad(x.w, y.w, grad_scale, alpha));
            }
            for (int i = (n4 << 2) + threadIdx.x; i < cnt; i += CL_THREADS) {
                const float G = proj_grad(g[off + i], r[off + i], grad_scale, alpha);
                ss = __builtin_fmaf(G, G, ss);
            }
        }
        const float t = block_sum(ss, sh);
        if (threadIdx.x == 0) chunk_sumsq[c] = t;
    }
}

// ... the projected gradient already carries grad_scale: the root is scaled only when the step did not project
__global__ __launch_bounds__(GN_THREADS) void grad_norm_finish_projected_kernel(const float* __restrict__ chunk_sumsq,
                                                                                const int* __restrict__ seg_chunk_begin, int nseg,
                                                                                float abs_scale, float max_norm,
                                                                                float* __restrict__ seg_norm,
                                                                                float* __restrict__ norm_state,
                                                                                const float* __restrict__ proj_state) {
    grad_norm_finish(chunk_sumsq, seg_chunk_begin, nseg, proj_state[3] != 0.f ? 1.f : abs_scale, max_norm, seg_norm, norm_state);
}

// The segmented AdamW on the projected gradient.  Per element of a live tensor (liveness is that of the task gradient g):
//   ge = g * grad_scale;   gp = violated ? ge - (alpha * r) : ge;   G = CLIP ? gp * coef : gp;   theta, m, v = AdamW(theta, G)
// with the explicit roundings of adamw1_rn, so that an un-projected step moves weights, moments, counters and the bf16 image
// exactly as adamw_seg_kernel does (r is then not read at all).
template <bool CLIP, bool TAIL>
__device__ __forceinline__ void adamw_proj1(float& p, float g, float r, float& m, float& v, bool violated, float alpha,
                                            const si_consts& k) {
    const float ge = mul_rn(g, k.grad_scale);
    const float gp = violated ? sub_rn(ge, mul_rn(alpha, r)) : ge;
    const float G = CLIP ? mul_rn(gp, k.coef) : gp;
    adamw1_rn<TAIL>(p, G, m, v, k.decay, k.omb1, k.b2, k.omb2, k.eps, k.step_size, k.inv_bc2_sqrt);
}

template <bool CLIP>
__global__ __launch_bounds__(CL_THREADS) void adamw_seg_proj_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                    float* __restrict__ m, float* __restrict__ v,
                                                                    const int4* __restrict__ table, int nchunks,
                                                                    const int* __restrict__ seg_active,
                                                                    const int* __restrict__ seg_step, const group_table groups,
                                                                    const int* __restrict__ seg_group, float b1, float b2, float eps,
                                                                    float grad_scale,
                                                                    unsigned short* __restrict__ shadow_bf16,
                                                                    const float* __restrict__ norm_state, int skip_nonfinite,
                                                                    const float* __restrict__ ref,
                                                                    const float* __restrict__ proj_state) {
    __shared__ float sh_c[2];
    float coef = 1.f;
    if (CLIP) {
        if (skip_nonfinite && norm_state[2] != 0.f) return;
        coef = norm_state[1];
    }
    const bool violated = proj_state[3] != 0.f;      // uniform over the launch
    const float alpha = proj_state[2];
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int4 e = table[c];
        if (!seg_active[e.z]) {           // workgroup-uniform: no task gradient -- untouched whatever r holds there
            if (shadow_bf16)
                for (int i = threadIdx.x; i < e.y; i += CL_THREADS) {
                    __hip_bfloat16 a = __float2bfloat16(p[e.x + i]);
                    shadow_bf16[e.x + i] = *reinterpret_cast<unsigned short*>(&a);
                }
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
        const si_consts k = {__builtin_fmaf(-lr, wd, 1.f), 1.f - b1, b2, 1.f - b2, eps, sh_c[0], sh_c[1], grad_scale, coef, 0.f};
        const int off = e.x, cnt = e.y, n4 = cnt >> 2;
        for (int q = threadIdx.x; q < n4; q += CL_THREADS) {
            float4 P = reinterpret_cast<float4*>(p + off)[q];
            const float4 G = reinterpret_cast<const float4*>(g + off)[q];
            float4 M = reinterpret_cast<float4*>(m + off)[q];
            float4 V = reinterpret_cast<float4*>(v + off)[q];
            float4 R = make_float4(0.f, 0.f, 0.f, 0.f);
            if (violated) R = reinterpret_cast<const float4*>(ref + off)[q];
            adamw_proj1<CLIP, false>(P.x, G.x, R.x, M.x, V.x, violated, alpha, k);
            adamw_proj1<CLIP, false>(P.y, G.y, R.y, M.y, V.y, violated, alpha, k);
            adamw_proj1<CLIP, false>(P.z, G.z, R.z, M.z, V.z, violated, alpha, k);
            adamw_proj1<CLIP, false>(P.w, G.w, R.w, M.w, V.w, violated, alpha, k);
            reinterpret_cast<float4*>(p + off)[q] = P;
            reinterpret_cast<float4*>(m + off)[q] = M;
            reinterpret_cast<float4*>(v + off)[q] = V;
            if (shadow_bf16) {
                __hip_bfloat16 a = __float2bfloat16(P.x), b = __float2bfloat16(P.y), cc = __float2bfloat16(P.z),
                               d = __float2bfloat16(P.w);
                ushort4 o;
                o.x = *reinterpret_cast<unsigned short*>(&a); o.y = *reinterpret_cast<unsigned short*>(&b);
                o.z = *reinterpret_cast<unsigned short*>(&cc); o.w = *reinterpret_cast<unsigned short*>(&d);
                reinterpret_cast<ushort4*>(shadow_bf16 + off)[q] = o;
            }
        }
        for (int i = (n4 << 2) + threadIdx.x; i < cnt; i += CL_THREADS) {
            float P = p[off + i], M = m[off + i], V = v[off + i];
            const float R = violated ? ref[off + i] : 0.f;
            adamw_proj1<CLIP, true>(P, g[off + i], R, M, V, violated, alpha, k);
            p[off + i] = P; m[off + i] = M; v[off + i] = V;
            if (shadow_bf16) { __hip_bfloat16 a = __float2bfloat16(P); shadow_bf16[off + i] = *reinterpret_cast<unsigned short*>(&a); }
        }
    }
}

__global__ void seg_step_advance_kernel(int* __restrict__ seg_active, int* __restrict__ seg_step, int nseg) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < nseg) { seg_step[s] += seg_active[s] ? 1 : 0; seg_active[s] = 0; }
}

// ... after a clipped step: a skipped step only clears the flags; counters = {clipped steps, skipped steps}
__global__ void seg_step_advance_clipped_kernel(int* __restrict__ seg_active, int* __restrict__ seg_step, int nseg,
                                                const float* __restrict__ norm_state, int skip_nonfinite,
                                                int* __restrict__ counters) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    const bool skipped = skip_nonfinite && norm_state[2] != 0.f;
    if (s < nseg) { seg_step[s] += (!skipped && seg_active[s]) ? 1 : 0; seg_active[s] = 0; }
    if (s == 0) {
        if (skipped) counters[1] += 1;
        else if (norm_state[1] < 1.f) counters[0] += 1;
    }
}

// ... after a projected step: norm_state / counters may both be NULL (nothing measured); proj_counters[0] counts the steps that
// projected, a skipped step not among them
__global__ void seg_step_advance_projected_kernel(int* __restrict__ seg_active, int* __restrict__ seg_step, int nseg,
                                                  const float* __restrict__ norm_state, int skip_nonfinite,
                                                  int* __restrict__ counters, const float* __restrict__ proj_state,
                                                  int* __restrict__ proj_counters) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    const bool skipped = norm_state && skip_nonfinite && norm_state[2] != 0.f;
    if (s < nseg) { seg_step[s] += (!skipped && seg_active[s]) ? 1 : 0; seg_active[s] = 0; }
    if (s == 0) {
        if (skipped) counters[1] += 1;
        else if (norm_state && norm_state[1] < 1.f) counters[0] += 1;
        if (!skipped && proj_state[3] != 0.f) proj_counters[0] += 1;
    }
}

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
//   gem_norm_kernel, adamw_seg_gem_kernel   proj_norm_kernel / adamw_seg_proj_kernel with g * s + sum_k v_k * r_k
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

__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

// acc = g * s, then acc += v_k * r_k for k ascending over the rows with v_k != 0: every product and sum rounded on its own
__device__ __forceinline__ float4 gem_grad4(float4 g, const float* __restrict__ refs, int64_t stride, int K, int64_t q4,
                                            const float* sh_v, float grad_scale) {
    float4 a = make_float4(mul_rn(g.x, grad_scale), mul_rn(g.y, grad_scale), mul_rn(g.z, grad_scale), mul_rn(g.w, grad_scale));
    for (int k = 0; k < K; ++k) {
        const float vk = sh_v[k];
        if (vk == 0.f) continue;                 // workgroup-uniform: the row is not read
        const float4 r = reinterpret_cast<const float4*>(refs + (int64_t)k * stride)[q4];
        a.x = add_rn(a.x, mul_rn(vk, r.x)); a.y = add_rn(a.y, mul_rn(vk, r.y));
        a.z = add_rn(a.z, mul_rn(vk, r.z)); a.w = add_rn(a.w, mul_rn(vk, r.w));
    }
    return a;
}

__device__ __forceinline__ float gem_grad1(float g, const float* __restrict__ refs, int64_t stride, int K, int64_t i,
                                           const float* sh_v, float grad_scale) {
    float a = mul_rn(g, grad_scale);
    for (int k = 0; k < K; ++k) {
        const float vk = sh_v[k];
        if (vk != 0.f) a = add_rn(a, mul_rn(vk, refs[(int64_t)k * stride + i]));
    }
    return a;
}

// proj_norm_kernel for GEM: un-projected, the raw sum of g^2 over every chunk (ia_grad_norm's first pass bit for bit);
// projected, the sum of G^2 over the chunks of live tensors, a dead tensor's chunk storing 0.
__global__ __launch_bounds__(CL_THREADS) void gem_norm_kernel(const float* __restrict__ g, const float* __restrict__ refs,
                                                              int64_t stride, int K, const int4* __restrict__ table, int nchunks,
                                                              const int* __restrict__ seg_active,
                                                              const float* __restrict__ gem_state, float grad_scale,
                                                              float* __restrict__ chunk_sumsq) {
    __shared__ float sh[CL_THREADS / 64];
    __shared__ float sh_v[GEM_MAX];
    const bool violated = gem_state[GEM_VIOLATED] != 0.f;
    if (threadIdx.x < GEM_MAX) sh_v[threadIdx.x] = gem_state[GEM_V + threadIdx.x];
    __syncthreads();
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int4 e = table[c];
        const int off = e.x, cnt = e.y, n4 = cnt >> 2;
        float ss = 0.f;
        if (!violated) {
            for (int q = threadIdx.x; q < n4; q += CL_THREADS) {
                const float4 x = reinterpret_cast<const float4*>(g + off)[q];
                ss = sumsq4_rn(ss, x.x, x.y, x.z, x.w);
            }
            for (int i = (n4 << 2) + threadIdx.x; i < cnt; i += CL_THREADS) ss = __builtin_fmaf(g[off + i], g[off + i], ss);
        } else if (!seg_active || seg_active[e.z]) {
            for (int q = threadIdx.x; q < n4; q += CL_THREADS) {
                const float4 G = gem_grad4(reinterpret_cast<const float4*>(g + off)[q], refs, stride, K, (off >> 2) + q, sh_v,
                                           grad_scale);
                ss = sumsq4_rn(ss, G.x, G.y, G.z, G.w);
            }
            for (int i = (n4 << 2) + threadIdx.x; i < cnt; i += CL_THREADS) {
                const float G = gem_grad1(g[off + i], refs, stride, K, off + i, sh_v, grad_scale);
                ss = __builtin_fmaf(G, G, ss);
            }
        }
        const float t = block_sum(ss, sh);
        if (threadIdx.x == 0) chunk_sumsq[c] = t;
    }
}

__global__ __launch_bounds__(GN_THREADS) void grad_norm_finish_gem_kernel(const float* __restrict__ chunk_sumsq,
                                                                          const int* __restrict__ seg_chunk_begin, int nseg,
                                                                          float abs_scale, float max_norm,
                                                                          float* __restrict__ seg_norm,
                                                                          float* __restrict__ norm_state,
                                                                          const float* __restrict__ gem_state) {
    grad_norm_finish(chunk_sumsq, seg_chunk_begin, nseg, gem_state[GEM_VIOLATED] != 0.f ? 1.f : abs_scale, max_norm, seg_norm,
                     norm_state);
}

// adamw_seg_proj_kernel with the K-row gradient: an un-projected step reads no row and is adamw_seg_kernel bit for bit
template <bool CLIP>
__global__ __launch_bounds__(CL_THREADS) void adamw_seg_gem_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                   float* __restrict__ m, float* __restrict__ v,
                                                                   const int4* __restrict__ table, int nchunks,
                                                                   const int* __restrict__ seg_active,
                                                                   const int* __restrict__ seg_step, const group_table groups,
                                                                   const int* __restrict__ seg_group, float b1, float b2, float eps,
                                                                   float grad_scale,
                                                                   unsigned short* __restrict__ shadow_bf16,
                                                                   const float* __restrict__ norm_state, int skip_nonfinite,
                                                                   const float* __restrict__ refs, int64_t stride, int ntasks,
                                                                   const float* __restrict__ gem_state) {
    __shared__ float sh_c[2];
    __shared__ float sh_v[GEM_MAX];
    float coef = 1.f;
    if (CLIP) {
        if (skip_nonfinite && norm_state[2] != 0.f) return;
        coef = norm_state[1];
    }
    const int K = gem_state[GEM_VIOLATED] != 0.f ? ntasks : 0;      // uniform over the launch; 0: no row is read
    if (threadIdx.x < GEM_MAX) sh_v[threadIdx.x] = gem_state[GEM_V + threadIdx.x];
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int4 e = table[c];
        if (!seg_active[e.z]) {           // workgroup-uniform: no task gradient -- untouched whatever the rows hold there
            if (shadow_bf16)
                for (int i = threadIdx.x; i < e.y; i += CL_THREADS) {
                    __hip_bfloat16 a = __float2bfloat16(p[e.x + i]);
                    shadow_bf16[e.x + i] = *reinterpret_cast<unsigned short*>(&a);
                }
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
        const si_consts k = {__builtin_fmaf(-lr, wd, 1.f), 1.f - b1, b2, 1.f - b2, eps, sh_c[0], sh_c[1], grad_scale, coef, 0.f};
        const int off = e.x, cnt = e.y, n4 = cnt >> 2;
        for (int q = threadIdx.x; q < n4; q += CL_THREADS) {
            float4 P = reinterpret_cast<float4*>(p + off)[q];
            float4 G = gem_grad4(reinterpret_cast<const float4*>(g + off)[q], refs, stride, K, (off >> 2) + q, sh_v, grad_scale);
            float4 M = reinterpret_cast<float4*>(m + off)[q];
            float4 V = reinterpret_cast<float4*>(v + off)[q];
            if (CLIP) { G.x = mul_rn(G.x, coef); G.y = mul_rn(G.y, coef); G.z = mul_rn(G.z, coef); G.w = mul_rn(G.w, coef); }
            adamw1_rn<false>(P.x, G.x, M.x, V.x, k.decay, k.omb1, k.b2, k.omb2, k.eps, k.step_size, k.inv_bc2_sqrt);
            adamw1_rn<false>(P.y, G.y, M.y, V.y, k.decay, k.omb1, k.b2, k.omb2, k.eps, k.step_size, k.inv_bc2_sqrt);
            adamw1_rn<false>(P.z, G.z, M.z, V.z, k.decay, k.omb1, k.b2, k.omb2, k.eps, k.step_size, k.inv_bc2_sqrt);
            adamw1_rn<false>(P.w, G.w, M.w, V.w, k.decay, k.omb1, k.b2, k.omb2, k.eps, k.step_size, k.inv_bc2_sqrt);
            reinterpret_cast<float4*>(p + off)[q] = P;
            reinterpret_cast<float4*>(m + off)[q] = M;
            reinterpret_cast<float4*>(v + off)[q] = V;
            if (shadow_bf16) {
                __hip_bfloat16 a = __float2bfloat16(P.x), b = __float2bfloat16(P.y), cc = __float2bfloat16(P.z),
                               d = __float2bfloat16(P.w);
                ushort4 o;
                o.x = *reinterpret_cast<unsigned short*>(&a); o.y = *reinterpret_cast<unsigned short*>(&b);
                o.z = *reinterpret_cast<unsigned short*>(&cc); o.w = *reinterpret_cast<unsigned short*>(&d);
                reinterpret_cast<ushort4*>(shadow_bf16 + off)[q] = o;
            }
        }
        for (int i = (n4 << 2) + threadIdx.x; i < cnt; i += CL_THREADS) {
            float P = p[off + i], M = m[off + i], V = v[off + i];
            float G = gem_grad1(g[off + i], refs, stride, K, off + i, sh_v, grad_scale);
            if (CLIP) G = mul_rn(G, coef);
            adamw1_rn<true>(P, G, M, V, k.decay, k.omb1, k.b2, k.omb2, k.eps, k.step_size, k.inv_bc2_sqrt);
            p[off + i] = P; m[off + i] = M; v[off + i] = V;
            if (shadow_bf16) { __hip_bfloat16 a = __float2bfloat16(P); shadow_bf16[off + i] = *reinterpret_cast<unsigned short*>(&a); }
        }
    }
}

// ... after a GEM step: gem_counters = {projected steps, unsolved steps}; a skipped step does not count as projected, and a
// step whose program could not be solved counts as unsolved whether or not it was skipped
__global__ void seg_step_advance_gem_kernel(int* __restrict__ seg_active, int* __restrict__ seg_step, int nseg,
                                            const float* __restrict__ norm_state, int skip_nonfinite,
                                            int* __restrict__ counters, const float* __restrict__ gem_state,
                                            int* __restrict__ gem_counters) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    const bool skipped = norm_state && skip_nonfinite && norm_state[2] != 0.f;
    if (s < nseg) { seg_step[s] += (!skipped && seg_active[s]) ? 1 : 0; seg_active[s] = 0; }
    if (s == 0) {
        if (skipped) counters[1] += 1;
        else if (norm_state && norm_state[1] < 1.f) counters[0] += 1;
        if (!skipped && gem_state[GEM_VIOLATED] != 0.f) gem_counters[0] += 1;
        if (gem_state[GEM_SOLVED] == 0.f) gem_counters[1] += 1;
    }
}

// ---- Piggyback (Mallya, Davis, Lazebnik 2018): a fixed backbone `base` and, per language, a binary mask over it that is
// trained through real-valued scores.  Per tensor a kind (workgroup-uniform per chunk, read inside the chunk loop as group_of is):
//   free    adamw_seg_kernel's arithmetic on theta (adamw1_rn restates it), so a free tensor moves as under the plain step
//   masked  ge = g * grad_scale [* coef];  gs = ge * base;  score, m, v = AdamW(score, gs) with weight decay 0 (decay factor 1);
//           theta = score >= threshold ? base : +0;  every product rounded on its own
//   frozen  nothing but the bf16 image
// A masked element moves 38 B (g, base, score, m, v in; score, m, v, theta and the bf16 image out), a free one 30 B.
constexpr int KIND_MASKED = IA_MASK_MASKED, KIND_FROZEN = IA_MASK_FROZEN;      // anything else is IA_MASK_FREE

__device__ __forceinline__ unsigned short bf16_bits(float x) {
    __hip_bfloat16 a = __float2bfloat16(x);
    return *reinterpret_cast<unsigned short*>(&a);
}

template <bool CLIP, bool TAIL>
__device__ __forceinline__ float adamw_mask1(float& s, float g, float base, float& m, float& v, float threshold,
                                             const si_consts& k) {
    const float ge = mul_rn(g, k.grad_scale);
    const float eff = CLIP ? mul_rn(ge, k.coef) : ge;           // eff_grad<true>'s two products
    adamw1_rn<TAIL>(s, mul_rn(eff, base), m, v, 1.f, k.omb1, k.b2, k.omb2, k.eps, k.step_size, k.inv_bc2_sqrt);
    return s >= threshold ? base : 0.f;
}

template <bool CLIP>
__global__ __launch_bounds__(CL_THREADS) void adamw_seg_masked_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                      float* __restrict__ m, float* __restrict__ v,
                                                                      const int4* __restrict__ table, int nchunks,
                                                                      const int* __restrict__ seg_active,
                                                                      const int* __restrict__ seg_step, const group_table groups,
                                                                      const int* __restrict__ seg_group, float b1, float b2,
                                                                      float eps, float grad_scale,
                                                                      unsigned short* __restrict__ shadow_bf16,
                                                                      const float* __restrict__ norm_state, int skip_nonfinite,
                                                                      const float* __restrict__ base, float* __restrict__ scores,
                                                                      const int* __restrict__ seg_kind, float threshold) {
    __shared__ float sh_c[2];
    float coef = 1.f;
    if (CLIP) {
        if (skip_nonfinite && norm_state[2] != 0.f) return;
        coef = norm_state[1];
    }
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int4 e = table[c];
        const int kind = seg_kind[e.z];                          // workgroup-uniform
        if (kind == KIND_FROZEN || !seg_active[e.z]) {           // never written / untouched: only the bf16 image is kept in step
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
        const si_consts k = {__builtin_fmaf(-lr, wd, 1.f), 1.f - b1, b2, 1.f - b2, eps, sh_c[0], sh_c[1], grad_scale, coef, 0.f};
        const int off = e.x, cnt = e.y, n4 = cnt >> 2;
        if (kind == KIND_MASKED) {
            for (int q = threadIdx.x; q < n4; q += CL_THREADS) {
                const float4 G = reinterpret_cast<const float4*>(g + off)[q];
                const float4 B = reinterpret_cast<const float4*>(base + off)[q];
                float4 S = reinterpret_cast<float4*>(scores + off)[q];
                float4 M = reinterpret_cast<float4*>(m + off)[q];
                float4 V = reinterpret_cast<float4*>(v + off)[q];
                float4 P;
                P.x = adamw_mask1<CLIP, false>(S.x, G.x, B.x, M.x, V.x, threshold, k);
                P.y = adamw_mask1<CLIP, false>(S.y, G.y, B.y, M.y, V.y, threshold, k);
                P.z = adamw_mask1<CLIP, false>(S.z, G.z, B.z, M.z, V.z, threshold, k);
                P.w = adamw_mask1<CLIP, false>(S.w, G.w, B.w, M.w, V.w, threshold, k);
                reinterpret_cast<float4*>(scores + off)[q] = S;
                reinterpret_cast<float4*>(m + off)[q] = M;
                reinterpret_cast<float4*>(v + off)[q] = V;
                reinterpret_cast<float4*>(p + off)[q] = P;
                if (shadow_bf16) {
                    ushort4 o;
                    o.x = bf16_bits(P.x); o.y = bf16_bits(P.y); o.z = bf16_bits(P.z); o.w = bf16_bits(P.w);
                    reinterpret_cast<ushort4*>(shadow_bf16 + off)[q] = o;
                }
            }
            for (int i = (n4 << 2) + threadIdx.x; i < cnt; i += CL_THREADS) {
                float S = scores[off + i], M = m[off + i], V = v[off + i];
                const float P = adamw_mask1<CLIP, true>(S, g[off + i], base[off + i], M, V, threshold, k);
                scores[off + i] = S; m[off + i] = M; v[off + i] = V; p[off + i] = P;
                if (shadow_bf16) shadow_bf16[off + i] = bf16_bits(P);
            }
            continue;
        }
        for (int q = threadIdx.x; q < n4; q += CL_THREADS) {    // free: adamw_seg_gem_kernel's un-projected path
            float4 P = reinterpret_cast<float4*>(p + off)[q];
            float4 G = reinterpret_cast<const float4*>(g + off)[q];
            float4 M = reinterpret_cast<float4*>(m + off)[q];
            float4 V = reinterpret_cast<float4*>(v + off)[q];
            G.x = mul_rn(G.x, grad_scale); G.y = mul_rn(G.y, grad_scale); G.z = mul_rn(G.z, grad_scale); G.w = mul_rn(G.w, grad_scale);
            if (CLIP) { G.x = mul_rn(G.x, coef); G.y = mul_rn(G.y, coef); G.z = mul_rn(G.z, coef); G.w = mul_rn(G.w, coef); }
            adamw1_rn<false>(P.x, G.x, M.x, V.x, k.decay, k.omb1, k.b2, k.omb2, k.eps, k.step_size, k.inv_bc2_sqrt);
            adamw1_rn<false>(P.y, G.y, M.y, V.y, k.decay, k.omb1, k.b2, k.omb2, k.eps, k.step_size, k.inv_bc2_sqrt);
            adamw1_rn<false>(P.z, G.z, M.z, V.z, k.decay, k.omb1, k.b2, k.omb2, k.eps, k.step_size, k.inv_bc2_sqrt);
            adamw1_rn<false>(P.w, G.w, M.w, V.w, k.decay, k.omb1, k.b2, k.omb2, k.eps, k.step_size, k.inv_bc2_sqrt);
            reinterpret_cast<float4*>(p + off)[q] = P;
            reinterpret_cast<float4*>(m + off)[q] = M;
            reinterpret_cast<float4*>(v + off)[q] = V;
            if (shadow_bf16) {
                ushort4 o;
                o.x = bf16_bits(P.x); o.y = bf16_bits(P.y); o.z = bf16_bits(P.z); o.w = bf16_bits(P.w);
                reinterpret_cast<ushort4*>(shadow_bf16 + off)[q] = o;
            }
        }
        for (int i = (n4 << 2) + threadIdx.x; i < cnt; i += CL_THREADS) {
            float P = p[off + i], M = m[off + i], V = v[off + i];
            float G = mul_rn(g[off + i], grad_scale);
            if (CLIP) G = mul_rn(G, coef);
            adamw1_rn<true>(P, G, M, V, k.decay, k.omb1, k.b2, k.omb2, k.eps, k.step_size, k.inv_bc2_sqrt);
            p[off + i] = P; m[off + i] = M; v[off + i] = V;
            if (shadow_bf16) shadow_bf16[off + i] = bf16_bits(P);
        }
    }
}

// ... after a masked step: a frozen tensor's counter never moves; norm_state / counters may both be NULL (nothing measured)
__global__ void seg_step_advance_masked_kernel(int* __restrict__ seg_active, int* __restrict__ seg_step, int nseg,
                                               const float* __restrict__ norm_state, int skip_nonfinite,
                                               int* __restrict__ counters, const int* __restrict__ seg_kind) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    const bool skipped = norm_state && skip_nonfinite && norm_state[2] != 0.f;
    if (s < nseg) { seg_step[s] += (!skipped && seg_active[s] && seg_kind[s] != KIND_FROZEN) ? 1 : 0; seg_active[s] = 0; }
    if (s == 0 && norm_state) {
        if (skipped) counters[1] += 1;
        else if (norm_state[1] < 1.f) counters[0] += 1;
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
            if (shadow_bf16) {
                ushort4 o;
                o.x = bf16_bits(P.x); o.y = bf16_bits(P.y); o.z = bf16_bits(P.z); o.w = bf16_bits(P.w);
                reinterpret_cast<ushort4*>(shadow_bf16 + off)[q] = o;
            }
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

inline int cap_grid(int64_t work_items, int per_block) {
    int64_t b = (work_items + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

inline group_table one_group(float lr, float weight_decay) {
    group_table t = {};
    t.n = 1;
    t.lr[0] = lr;
    t.weight_decay[0] = weight_decay;
    return t;
}

// The launches of the four kinds of segmented step, shared by their entry points (one group, seg_group NULL) and by
// ia_adamw_step_segmented_grouped.  Arguments are validated by the callers.
struct step_head {
    float *theta; const float* grad; float *exp_avg, *exp_avg_sq;
    const int4* table; int nchunks; int32_t *seg_active, *seg_step; int nseg, all_active;
    float b1, b2, eps, grad_scale; unsigned short* shadow;
};

inline bool step_head_ok(const float* theta, const float* grad, const float* exp_avg, const float* exp_avg_sq,
                         const int32_t* chunk_table, int nchunks, const int32_t* seg_active, const int32_t* seg_step, int nseg,
                         const void* shadow_bf16) {
    if (!theta || !grad || !exp_avg || !exp_avg_sq || !chunk_table || !seg_active || !seg_step || nchunks <= 0 || nseg <= 0)
        return false;
    return ia_is_aligned(theta, 16) && ia_is_aligned(grad, 16) && ia_is_aligned(exp_avg, 16) && ia_is_aligned(exp_avg_sq, 16) &&
           ia_is_aligned(chunk_table, 16) && (!shadow_bf16 || ia_is_aligned(shadow_bf16, 8));
}

inline bool si_operands_ok(const float* norm_state, const int32_t* counters, const float* path_w, const float* omega,
                           const float* theta_star) {
    if (!path_w || (norm_state == nullptr) != (counters == nullptr) || (omega == nullptr) != (theta_star == nullptr)) return false;
    return ia_is_aligned(path_w, 16) && (!omega || (ia_is_aligned(omega, 16) && ia_is_aligned(theta_star, 16)));
}

inline bool proj_operands_ok(const float* norm_state, const int32_t* counters, const float* ref, const float* proj_state,
                             const int32_t* proj_counters) {
    if (!ref || !proj_state || !proj_counters || (norm_state == nullptr) != (counters == nullptr)) return false;
    return ia_is_aligned(ref, 16) && ia_is_aligned(proj_state, 4) && ia_is_aligned(proj_counters, 4);
}

inline int step_grid(const step_head& h) { return h.nchunks < 2048 ? h.nchunks : 2048; }

inline bool mark_all_active(const step_head& h, hipStream_t st) {   // 0x01010101: non-zero
    return hipMemsetAsync(h.seg_active, 1, (size_t)h.nseg * sizeof(int32_t), st) == hipSuccess;
}

inline void launch_activity(const step_head& h, hipStream_t st) {
    hipLaunchKernelGGL(seg_activity_kernel<false>, dim3(step_grid(h)), dim3(CL_THREADS), 0, st, h.grad, h.table, h.nchunks,
                       h.seg_active, (float*)nullptr);
}

inline void launch_advance(const step_head& h, const float* norm_state, int skip_nonfinite, int32_t* counters, hipStream_t st) {
    const dim3 grid((h.nseg + 255) / 256), block(256);
    if (norm_state)
        hipLaunchKernelGGL(seg_step_advance_clipped_kernel, grid, block, 0, st, h.seg_active, h.seg_step, h.nseg, norm_state,
                           skip_nonfinite, counters);
    else
        hipLaunchKernelGGL(seg_step_advance_kernel, grid, block, 0, st, h.seg_active, h.seg_step, h.nseg);
}

// plain (norm_state NULL: the activity pass runs here unless all_active) or clipped (ia_grad_norm has set the flags)
int run_step(const step_head& h, const group_table& gt, const int32_t* seg_group, const float* norm_state, int skip_nonfinite,
             int32_t* counters, hipStream_t st) {
    if (h.all_active) {
        if (!mark_all_active(h, st)) return IA_LAUNCH_FAILED;
    } else if (!norm_state) {
        launch_activity(h, st);
    }
    auto kernel = norm_state ? adamw_seg_kernel<true> : adamw_seg_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(step_grid(h)), dim3(CL_THREADS), 0, st, h.theta, h.grad, h.exp_avg, h.exp_avg_sq, h.table,
                       h.nchunks, h.seg_active, h.seg_step, gt, seg_group, h.b1, h.b2, h.eps, h.grad_scale, h.shadow, norm_state,
                       skip_nonfinite);
    launch_advance(h, norm_state, skip_nonfinite, counters, st);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}

int run_step_si(const step_head& h, const group_table& gt, const int32_t* seg_group, const float* norm_state, int skip_nonfinite,
                int32_t* counters, float* path_w, const float* omega, const float* theta_star, float penalty_coef,
                hipStream_t st) {
    const bool clip = norm_state != nullptr, pen = omega != nullptr;
    if (h.all_active) {
        if (!mark_all_active(h, st)) return IA_LAUNCH_FAILED;
    } else if (!clip) {   // with norm_state, ia_grad_norm's first pass has set the flags
        launch_activity(h, st);
    }
    const float c2 = 2.f * penalty_coef;
    auto kernel = clip ? (pen ? adamw_seg_si_kernel<true, true> : adamw_seg_si_kernel<true, false>)
                       : (pen ? adamw_seg_si_kernel<false, true> : adamw_seg_si_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3(step_grid(h)), dim3(CL_THREADS), 0, st, h.theta, h.grad, h.exp_avg, h.exp_avg_sq, h.table,
                       h.nchunks, h.seg_active, h.seg_step, gt, seg_group, h.b1, h.b2, h.eps, h.grad_scale, h.shadow, norm_state,
                       skip_nonfinite, path_w, omega, theta_star, c2);
    launch_advance(h, norm_state, skip_nonfinite, counters, st);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}

int run_step_projected(const step_head& h, const group_table& gt, const int32_t* seg_group, const float* norm_state,
                       int skip_nonfinite, int32_t* counters, const float* ref, const float* proj_state, int32_t* proj_counters,
                       hipStream_t st) {
    if (h.all_active)   // otherwise ia_agem_dots has set the flags from the task gradient
        if (!mark_all_active(h, st)) return IA_LAUNCH_FAILED;
    auto kernel = norm_state ? adamw_seg_proj_kernel<true> : adamw_seg_proj_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(step_grid(h)), dim3(CL_THREADS), 0, st, h.theta, h.grad, h.exp_avg, h.exp_avg_sq, h.table,
                       h.nchunks, h.seg_active, h.seg_step, gt, seg_group, h.b1, h.b2, h.eps, h.grad_scale, h.shadow, norm_state,
                       skip_nonfinite, ref, proj_state);
    hipLaunchKernelGGL(seg_step_advance_projected_kernel, dim3((h.nseg + 255) / 256), dim3(256), 0, st, h.seg_active, h.seg_step,
                       h.nseg, norm_state, skip_nonfinite, counters, proj_state, proj_counters);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}

inline bool gem_operands_ok(const float* refs, int64_t stride, int ntasks, const float* gem_state) {
    if (!refs || !gem_state || ntasks < 1 || ntasks > GEM_MAX || stride <= 0 || (stride & 3)) return false;
    return ia_is_aligned(refs, 16) && ia_is_aligned(gem_state, 4);
}

int run_step_gem(const step_head& h, const group_table& gt, const int32_t* seg_group, const float* norm_state, int skip_nonfinite,
                 int32_t* counters, const float* refs, int64_t stride, int ntasks, const float* gem_state, int32_t* gem_counters,
                 hipStream_t st) {
    if (h.all_active)   // otherwise ia_gem_dots has set the flags from the task gradient
        if (!mark_all_active(h, st)) return IA_LAUNCH_FAILED;
    auto kernel = norm_state ? adamw_seg_gem_kernel<true> : adamw_seg_gem_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(step_grid(h)), dim3(CL_THREADS), 0, st, h.theta, h.grad, h.exp_avg, h.exp_avg_sq, h.table,
                       h.nchunks, h.seg_active, h.seg_step, gt, seg_group, h.b1, h.b2, h.eps, h.grad_scale, h.shadow, norm_state,
                       skip_nonfinite, refs, stride, ntasks, gem_state);
    hipLaunchKernelGGL(seg_step_advance_gem_kernel, dim3((h.nseg + 255) / 256), dim3(256), 0, st, h.seg_active, h.seg_step,
                       h.nseg, norm_state, skip_nonfinite, counters, gem_state, gem_counters);
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
    if (!step_head_ok(theta, grad, exp_avg, exp_avg_sq, chunk_table, nchunks, seg_active, seg_step, nseg, shadow_bf16))
        return IA_INVALID_VALUE;
    const step_head h = {theta, grad, exp_avg, exp_avg_sq, (const int4*)chunk_table, nchunks, seg_active, seg_step, nseg, all_active,
                         beta1, beta2, eps, grad_scale, (unsigned short*)shadow_bf16};
    return run_step(h, one_group(lr, weight_decay), nullptr, nullptr, 0, nullptr, (hipStream_t)stream);
}

extern "C" size_t ia_grad_norm_workspace_bytes(int nchunks) { return nchunks > 0 ? (size_t)nchunks * sizeof(float) : 0; }

extern "C" int ia_grad_norm(const float* grad, const int32_t* chunk_table, int nchunks, const int32_t* seg_chunk_begin, int nseg,
                            float grad_scale, float max_norm, int32_t* seg_active, float* seg_norm, float* norm_state,
                            void* workspace, size_t workspace_bytes, ia_stream_t stream) {
    if (!grad || !chunk_table || !seg_chunk_begin || !seg_norm || !norm_state || !workspace || nchunks <= 0 || nseg <= 0)
        return IA_INVALID_VALUE;
    if (!ia_is_aligned(grad, 16) || !ia_is_aligned(chunk_table, 16) || !ia_is_aligned(workspace, 4)) return IA_INVALID_VALUE;
    if (workspace_bytes < ia_grad_norm_workspace_bytes(nchunks)) return IA_WORKSPACE_TOO_SMALL;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(seg_activity_kernel<true>, dim3(nchunks < 2048 ? nchunks : 2048), dim3(CL_THREADS), 0, st, grad,
                       (const int4*)chunk_table, nchunks, seg_active, (float*)workspace);
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(GN_THREADS), 0, st, (const float*)workspace, seg_chunk_begin, nseg,
                       fabsf(grad_scale), max_norm, seg_norm, norm_state);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}

extern "C" int ia_adamw_step_segmented_clipped(float* theta, const float* grad, float* exp_avg, float* exp_avg_sq,
                                               const int32_t* chunk_table, int nchunks, int32_t* seg_active, int32_t* seg_step,
                                               int nseg, int all_active, float lr, float beta1, float beta2, float eps,
                                               float weight_decay, float grad_scale, void* shadow_bf16, const float* norm_state,
                                               int skip_nonfinite, int32_t* counters, ia_stream_t stream) {
    if (!norm_state || !counters ||
        !step_head_ok(theta, grad, exp_avg, exp_avg_sq, chunk_table, nchunks, seg_active, seg_step, nseg, shadow_bf16))
        return IA_INVALID_VALUE;
    const step_head h = {theta, grad, exp_avg, exp_avg_sq, (const int4*)chunk_table, nchunks, seg_active, seg_step, nseg, all_active,
                         beta1, beta2, eps, grad_scale, (unsigned short*)shadow_bf16};
    return run_step(h, one_group(lr, weight_decay), nullptr, norm_state, skip_nonfinite, counters, (hipStream_t)stream);
}

extern "C" int ia_adamw_step_segmented_si(float* theta, const float* grad, float* exp_avg, float* exp_avg_sq,
                                          const int32_t* chunk_table, int nchunks, int32_t* seg_active, int32_t* seg_step, int nseg,
                                          int all_active, float lr, float beta1, float beta2, float eps, float weight_decay,
                                          float grad_scale, void* shadow_bf16, const float* norm_state, int skip_nonfinite,
                                          int32_t* counters, float* path_w, const float* omega, const float* theta_star,
                                          float penalty_coef, ia_stream_t stream) {
    if (!step_head_ok(theta, grad, exp_avg, exp_avg_sq, chunk_table, nchunks, seg_active, seg_step, nseg, shadow_bf16) ||
        !si_operands_ok(norm_state, counters, path_w, omega, theta_star))
        return IA_INVALID_VALUE;
    const step_head h = {theta, grad, exp_avg, exp_avg_sq, (const int4*)chunk_table, nchunks, seg_active, seg_step, nseg, all_active,
                         beta1, beta2, eps, grad_scale, (unsigned short*)shadow_bf16};
    return run_step_si(h, one_group(lr, weight_decay), nullptr, norm_state, skip_nonfinite, counters, path_w, omega, theta_star,
                       penalty_coef, (hipStream_t)stream);
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
    if (!grad || !chunk_table || !seg_chunk_begin || !seg_norm || !norm_state || !workspace || !ref || !proj_state ||
        nchunks <= 0 || nseg <= 0)
        return IA_INVALID_VALUE;
    if (!ia_is_aligned(grad, 16) || !ia_is_aligned(ref, 16) || !ia_is_aligned(chunk_table, 16) || !ia_is_aligned(workspace, 4) ||
        !ia_is_aligned(proj_state, 4))
        return IA_INVALID_VALUE;
    if (workspace_bytes < ia_grad_norm_workspace_bytes(nchunks)) return IA_WORKSPACE_TOO_SMALL;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(proj_norm_kernel, dim3(nchunks < 2048 ? nchunks : 2048), dim3(CL_THREADS), 0, st, grad, ref,
                       (const int4*)chunk_table, nchunks, seg_active, proj_state, grad_scale, (float*)workspace);
    hipLaunchKernelGGL(grad_norm_finish_projected_kernel, dim3(1), dim3(GN_THREADS), 0, st, (const float*)workspace,
                       seg_chunk_begin, nseg, fabsf(grad_scale), max_norm, seg_norm, norm_state, proj_state);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}

extern "C" int ia_adamw_step_segmented_projected(float* theta, const float* grad, float* exp_avg, float* exp_avg_sq,
                                                 const int32_t* chunk_table, int nchunks, int32_t* seg_active, int32_t* seg_step,
                                                 int nseg, int all_active, float lr, float beta1, float beta2, float eps,
                                                 float weight_decay, float grad_scale, void* shadow_bf16, const float* norm_state,
                                                 int skip_nonfinite, int32_t* counters, const float* ref, const float* proj_state,
                                                 int32_t* proj_counters, ia_stream_t stream) {
    if (!step_head_ok(theta, grad, exp_avg, exp_avg_sq, chunk_table, nchunks, seg_active, seg_step, nseg, shadow_bf16) ||
        !proj_operands_ok(norm_state, counters, ref, proj_state, proj_counters))
        return IA_INVALID_VALUE;
    const step_head h = {theta, grad, exp_avg, exp_avg_sq, (const int4*)chunk_table, nchunks, seg_active, seg_step, nseg, all_active,
                         beta1, beta2, eps, grad_scale, (unsigned short*)shadow_bf16};
    return run_step_projected(h, one_group(lr, weight_decay), nullptr, norm_state, skip_nonfinite, counters, ref, proj_state,
                              proj_counters, (hipStream_t)stream);
}

// Any of the four steps with per-group lr / weight_decay: the operands that are present select the step.
extern "C" int ia_adamw_step_segmented_grouped(float* theta, const float* grad, float* exp_avg, float* exp_avg_sq,
                                               const int32_t* chunk_table, int nchunks, int32_t* seg_active, int32_t* seg_step,
                                               int nseg, int all_active, float beta1, float beta2, float eps, float grad_scale,
                                               void* shadow_bf16, const int32_t* seg_group, int ngroups, const float* group_lr,
                                               const float* group_weight_decay, const float* norm_state, int skip_nonfinite,
                                               int32_t* counters, float* path_w, const float* omega, const float* theta_star,
                                               float penalty_coef, const float* ref, const float* proj_state,
                                               int32_t* proj_counters, ia_stream_t stream) {
    if (!step_head_ok(theta, grad, exp_avg, exp_avg_sq, chunk_table, nchunks, seg_active, seg_step, nseg, shadow_bf16))
        return IA_INVALID_VALUE;
    if (ngroups < 1 || ngroups > IA_MAX_PARAM_GROUPS || !group_lr || !group_weight_decay || (ngroups > 1 && !seg_group) ||
        (seg_group && !ia_is_aligned(seg_group, 4)))
        return IA_INVALID_VALUE;
    const bool si = path_w || omega || theta_star, proj = ref || proj_state || proj_counters;
    if ((si && proj) || (norm_state == nullptr) != (counters == nullptr)) return IA_INVALID_VALUE;
    if (si && !si_operands_ok(norm_state, counters, path_w, omega, theta_star)) return IA_INVALID_VALUE;
    if (proj && !proj_operands_ok(norm_state, counters, ref, proj_state, proj_counters)) return IA_INVALID_VALUE;
    group_table gt = {};
    gt.n = ngroups;
    for (int k = 0; k < ngroups; ++k) { gt.lr[k] = group_lr[k]; gt.weight_decay[k] = group_weight_decay[k]; }
    const step_head h = {theta, grad, exp_avg, exp_avg_sq, (const int4*)chunk_table, nchunks, seg_active, seg_step, nseg, all_active,
                         beta1, beta2, eps, grad_scale, (unsigned short*)shadow_bf16};
    hipStream_t st = (hipStream_t)stream;
    if (proj) return run_step_projected(h, gt, seg_group, norm_state, skip_nonfinite, counters, ref, proj_state, proj_counters, st);
    if (si)
        return run_step_si(h, gt, seg_group, norm_state, skip_nonfinite, counters, path_w, omega, theta_star, penalty_coef, st);
    return run_step(h, gt, seg_group, norm_state, skip_nonfinite, counters, st);
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
    if (!grad || !chunk_table || !seg_chunk_begin || !seg_norm || !norm_state || !workspace || nchunks <= 0 || nseg <= 0 ||
        !gem_operands_ok(refs, stride, ntasks, gem_state))
        return IA_INVALID_VALUE;
    if (!ia_is_aligned(grad, 16) || !ia_is_aligned(chunk_table, 16) || !ia_is_aligned(workspace, 4)) return IA_INVALID_VALUE;
    if (workspace_bytes < ia_grad_norm_workspace_bytes(nchunks)) return IA_WORKSPACE_TOO_SMALL;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(gem_norm_kernel, dim3(nchunks < 2048 ? nchunks : 2048), dim3(CL_THREADS), 0, st, grad, refs, stride, ntasks,
                       (const int4*)chunk_table, nchunks, seg_active, gem_state, grad_scale, (float*)workspace);
    hipLaunchKernelGGL(grad_norm_finish_gem_kernel, dim3(1), dim3(GN_THREADS), 0, st, (const float*)workspace, seg_chunk_begin,
                       nseg, fabsf(grad_scale), max_norm, seg_norm, norm_state, gem_state);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}

extern "C" int ia_adamw_step_segmented_gem(float* theta, const float* grad, float* exp_avg, float* exp_avg_sq,
                                           const int32_t* chunk_table, int nchunks, int32_t* seg_active, int32_t* seg_step, int nseg,
                                           int all_active, float beta1, float beta2, float eps, float grad_scale, void* shadow_bf16,
                                           const int32_t* seg_group, int ngroups, const float* group_lr,
                                           const float* group_weight_decay, const float* norm_state, int skip_nonfinite,
                                           int32_t* counters, const float* refs, int64_t stride, int ntasks, const float* gem_state,
                                           int32_t* gem_counters, ia_stream_t stream) {
    if (!step_head_ok(theta, grad, exp_avg, exp_avg_sq, chunk_table, nchunks, seg_active, seg_step, nseg, shadow_bf16))
        return IA_INVALID_VALUE;
    if (ngroups < 1 || ngroups > IA_MAX_PARAM_GROUPS || !group_lr || !group_weight_decay || (ngroups > 1 && !seg_group) ||
        (seg_group && !ia_is_aligned(seg_group, 4)))
        return IA_INVALID_VALUE;
    if ((norm_state == nullptr) != (counters == nullptr) || !gem_counters || !ia_is_aligned(gem_counters, 4) ||
        !gem_operands_ok(refs, stride, ntasks, gem_state))
        return IA_INVALID_VALUE;
    group_table gt = {};
    gt.n = ngroups;
    for (int k = 0; k < ngroups; ++k) { gt.lr[k] = group_lr[k]; gt.weight_decay[k] = group_weight_decay[k]; }
    const step_head h = {theta, grad, exp_avg, exp_avg_sq, (const int4*)chunk_table, nchunks, seg_active, seg_step, nseg, all_active,
                         beta1, beta2, eps, grad_scale, (unsigned short*)shadow_bf16};
    return run_step_gem(h, gt, seg_group, norm_state, skip_nonfinite, counters, refs, stride, ntasks, gem_state, gem_counters,
                        (hipStream_t)stream);
}

extern "C" int ia_adamw_step_segmented_masked(float* theta, const float* grad, float* exp_avg, float* exp_avg_sq,
                                              const int32_t* chunk_table, int nchunks, int32_t* seg_active, int32_t* seg_step,
                                              int nseg, int all_active, float beta1, float beta2, float eps, float grad_scale,
                                              void* shadow_bf16, const int32_t* seg_group, int ngroups, const float* group_lr,
                                              const float* group_weight_decay, const float* norm_state, int skip_nonfinite,
                                              int32_t* counters, const float* base, float* scores, const int32_t* seg_kind,
                                              float threshold, ia_stream_t stream) {
    if (!step_head_ok(theta, grad, exp_avg, exp_avg_sq, chunk_table, nchunks, seg_active, seg_step, nseg, shadow_bf16))
        return IA_INVALID_VALUE;
    if (ngroups < 1 || ngroups > IA_MAX_PARAM_GROUPS || !group_lr || !group_weight_decay || (ngroups > 1 && !seg_group) ||
        (seg_group && !ia_is_aligned(seg_group, 4)))
        return IA_INVALID_VALUE;
    if ((norm_state == nullptr) != (counters == nullptr) || !base || !scores || !seg_kind || !ia_is_aligned(base, 16) ||
        !ia_is_aligned(scores, 16) || !ia_is_aligned(seg_kind, 4))
        return IA_INVALID_VALUE;
    group_table gt = {};
    gt.n = ngroups;
    for (int k = 0; k < ngroups; ++k) { gt.lr[k] = group_lr[k]; gt.weight_decay[k] = group_weight_decay[k]; }
    const step_head h = {theta, grad, exp_avg, exp_avg_sq, (const int4*)chunk_table, nchunks, seg_active, seg_step, nseg, all_active,
                         beta1, beta2, eps, grad_scale, (unsigned short*)shadow_bf16};
    hipStream_t st = (hipStream_t)stream;
    if (h.all_active) {
        if (!mark_all_active(h, st)) return IA_LAUNCH_FAILED;
    } else if (!norm_state) {   // with norm_state, ia_grad_norm's first pass has set the flags
        launch_activity(h, st);
    }
    auto kernel = norm_state ? adamw_seg_masked_kernel<true> : adamw_seg_masked_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(step_grid(h)), dim3(CL_THREADS), 0, st, h.theta, h.grad, h.exp_avg, h.exp_avg_sq, h.table,
                       h.nchunks, h.seg_active, h.seg_step, gt, seg_group, h.b1, h.b2, h.eps, h.grad_scale, h.shadow, norm_state,
                       skip_nonfinite, base, scores, seg_kind, threshold);
    hipLaunchKernelGGL(seg_step_advance_masked_kernel, dim3((h.nseg + 255) / 256), dim3(256), 0, st, h.seg_active, h.seg_step,
                       h.nseg, norm_state, skip_nonfinite, counters, seg_kind);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
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
