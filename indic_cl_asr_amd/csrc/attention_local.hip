// Local (windowed) relative-position multi-head self-attention forward: the key-tile loop of attention_flash.hip restricted to
// the band |i - j| <= w (gfx950).
//
//   ctx[b,i,h,:] = sum_j softmax_j( ((q_i+u_h).k_j + (q_i+v_h).p_h[w-i+j]) / sqrt(dk) ) v_j ,   |i - j| <= w, j < len_b
//
// RelPositionMultiHeadAttentionLongformer.forward A/parts/submodules/multi_head_attention.py:253-470 with
// LocalAttRelPositionalEncoding (:982-1026) for a symmetric window [w, w] and no global tokens: the sliding-chunk matmuls and
// their diagonal bookkeeping are this band, the position table's row r holds relative position w - r (2w + 1 rows), padded
// queries give zero context.  Asymmetric windows are not offered: the reference adds their position term to the wrong columns.
//
// Workgroup, LDS stage, fragments, band block, scores, online softmax and dropout hash are those of relpos_flash_fwd_kernel
// (attention_flash.h's vocabulary; the same operation order, so a window >= T - 1 gives the full kernel's bits).  What differs:
//   - query tile I0 walks only the key tiles that intersect [I0 - w, I0 + 63 + w] and lie below len: 1 + 2 ceil(w / 64) tiles
//     at the most (3 at w = 64), whatever T is; the one-stage prefetch follows that range;
//   - the staged position rows are w - I0 - 63 + j0 .. + 127 clamped to [0, 2w]: clamped rows give finite band values for keys
//     outside the window, which the band mask removes BEFORE the row maximum;
//   - a processed tile may hold no admissible key for a query (the tile left of the diagonal at a small w, queries >= len):
//     running and new maximum are then both -inf, so the exponentials are taken against 0 instead (exp2(-inf) = 0, no NaN);
//   - the mask-free score branch is per wave: the tile lies inside the window of each of the wave's 16 queries and below len.
// The host reduces a window beyond T - 1 to T - 1 by advancing the table pointer (row r of the 2w+1 table is row
// r - (w - w') of the 2w'+1 one), so the kernel's index arithmetic never sees a window larger than T.  The optional lse is the
// full kernel's (natural-log log-sum-exp per query, 0 for padded queries): attention_local_bwd.hip recomputes P = exp(s - lse).
#include "attention_flash.h"

namespace {

constexpr int FL_KT = 64;                              // keys per tile
constexpr int FL_STAGE = 2 * FA_T64 + FA_PBUF;         // K | V | P = 32 KB, the forward's stage
constexpr int FL_SR_BYTES = 16 * FA_SR_LD * 2;
constexpr int FL_LDS = FL_STAGE + 4 * FL_SR_BYTES;     // 46 080 B: three workgroups per CU

struct FlArgs {
    const __bf16* qkv; const __bf16* pl; const float* bias_u; const float* bias_v; const int64_t* lens;
    __bf16* ctx; int B, T, H, dk, w; float scale; unsigned seed, thr; float keep_scale;
    float* lse;   // optional [B*H, T], as relpos_flash_fwd_kernel writes it
};

template <bool DK64>
__global__ __launch_bounds__(FA_THREADS, 3) void relpos_local_fwd_kernel(FlArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, q4 = lane >> 4;
    const int T = a.T, H = a.H, dk = a.dk, d = H * dk, w = a.w;   // 0 <= w <= T - 1
    const FaWg wg = fa_wg(a.B, T, H, a.lens);
    if (wg.len < 0) return;
    const int bh = wg.bh, h = wg.h, b = wg.b, len = wg.len;
    const int I0 = wg.tile * 64;
    const int iw = I0 + wave * 16;
    const int iq = iw + c;                               // this lane's query
    __bf16* orow = a.ctx + ((size_t)b * T + (iq < T ? iq : T - 1)) * d + h * dk;
    if (I0 >= len) {                                     // workgroup-uniform: only padded queries -> zero context
        if (iq < T) {
            for (int mt = 0; mt < 4; ++mt) fa_store_head4(orow, mt, q4, dk, (f4){0.f, 0.f, 0.f, 0.f});
            if (a.lse && q4 == 0) a.lse[(size_t)bh * T + iq] = 0.f;
        }
        return;
    }
    unsigned char* sR = smem + FL_STAGE + wave * FL_SR_BYTES;

    bf8 Qu[2], Qv[2];
    {
        const int iqc = iq < T ? iq : T - 1;
        const __bf16* qrow = a.qkv + ((size_t)b * T + iqc) * (3 * d) + h * dk;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) fa_query_frags<DK64>(qrow, a.bias_u, a.bias_v, h, dk, ks, q4, Qu[ks], Qv[ks]);
    }

    FlKvpStage<DK64> stage(a.qkv, a.pl, smem, b, h, T, d, dk, I0, w, tid);

    // ---- key tiles of this query tile: those that hold a key of [max(I0 - w, 0), min(I0 + 63 + w, len - 1)].  Both ends are
    // non-negative (I0 < len here), so the divisions are plain; the first end is <= I0 <= the second.
    const int jlo = I0 - w > 0 ? I0 - w : 0;
    const int jhi = I0 + 63 + w < len - 1 ? I0 + 63 + w : len - 1;
    const int t_lo = jlo / FL_KT, t_hi = jhi / FL_KT;
    stage.fetch(t_lo);
    stage.commit();
    __syncthreads();

    f4 O[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) O[mt] = (f4){0.f, 0.f, 0.f, 0.f};
    float m_run = IA_NEG_INF, l_run = 0.f;
    const float scale2 = a.scale * 1.44269504088896341f;

    for (int t = t_lo; t <= t_hi; ++t) {
        const unsigned char* sK = smem;
        const unsigned char* sV = sK + FA_T64;
        const unsigned char* sP = sK + 2 * FA_T64;
        if (t < t_hi) stage.fetch(t + 1);
        const int j0 = t * FL_KT;
        fa_band_to_strip(sP, sR, (3 - wave) * 16, Qv, c, q4);
        f4 S[4];
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
            S[jt] = (f4){0.f, 0.f, 0.f, 0.f};
            const int row = jt * 16 + c;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
                S[jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa_frag(sK, row, ks, q4), Qu[ks], S[jt], 0, 0, 0);
        }
        // ---- scores as in the full kernel; mask-free (wave-uniform) when the whole tile is below len and inside the window of
        // every query iw .. iw + 15 of this wave, else masked by |i - j| <= w && j < len before the maximum
        float tmax = IA_NEG_INF;
        if (j0 + FL_KT <= len && j0 >= iw + 15 - w && j0 + FL_KT - 1 <= iw + w) {
#pragma unroll
            for (int jt = 0; jt < 4; ++jt) {
                union { uint2 u; __bf16 e[4]; } bd;
                bd.u = *reinterpret_cast<const uint2*>(sR + (c * FA_SR_LD + jt * 16 + q4 * 4 + 16) * 2);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float s = (S[jt][r] + (float)bd.e[r]) * scale2;
                    S[jt][r] = s;
                    tmax = fmaxf(tmax, s);
                }
            }
        } else {
            const int kmin = iq - w, kmax = iq + w < len - 1 ? iq + w : len - 1;   // this query's admissible keys
#pragma unroll
            for (int jt = 0; jt < 4; ++jt) {
                union { uint2 u; __bf16 e[4]; } bd;
                bd.u = *reinterpret_cast<const uint2*>(sR + (c * FA_SR_LD + jt * 16 + q4 * 4 + 16) * 2);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = j0 + jt * 16 + q4 * 4 + r;
                    const float s = (j >= kmin && j <= kmax) ? (S[jt][r] + (float)bd.e[r]) * scale2 : IA_NEG_INF;
                    S[jt][r] = s;
                    tmax = fmaxf(tmax, s);
                }
            }
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float m_new = fmaxf(m_run, tmax);
        // no admissible key for this query so far: -inf - -inf would be NaN, so the exponentials are taken against 0
        // (every one is exp2(-inf) = 0); m_run stays -inf until a key arrives
        const float m_ref = (m_new == IA_NEG_INF) ? 0.f : m_new;
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_ref);
        m_run = m_new;
        float psum = 0.f;
        bf8 Pf[2];
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
            unsigned rnd4 = 0;
            if (a.thr > 0) rnd4 = fa_keep_rand4(a.seed, bh, T, iq, (j0 + jt * 16 + q4 * 4) >> 2);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float p = __builtin_amdgcn_exp2f(S[jt][r] - m_ref);
                psum += p;
                if (a.thr > 0) p = (((rnd4 >> (8 * r)) & 0xFFu) >= a.thr) ? p : 0.f;
                Pf[jt >> 1][(jt & 1) * 4 + r] = (__bf16)p;
            }
        }
        l_run = l_run * alpha + psum;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) O[mt][r] *= alpha;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const int qq = c >> 2, p = c & 3;
                const int rowA = kk * 32 + q4 * 4 + qq;
                const bf8 vf = fa_tr_pair(sV, rowA, rowA + 16, mt * 2 + (p >> 1), p & 1);
                O[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, Pf[kk], O[mt], 0, 0, 0);
            }
        __syncthreads();                      // every wave is done with the stage
        if (t < t_hi) {
            stage.commit();
            __syncthreads();
        }
    }
    l_run += __shfl_xor(l_run, 16, 64);
    l_run += __shfl_xor(l_run, 32, 64);
    if (iq < T) {
        if (a.lse && q4 == 0) a.lse[(size_t)bh * T + iq] = (iq < len && l_run > 0.f) ? (m_run + __builtin_amdgcn_logf(l_run)) * 0.69314718055994531f : 0.f;
        const float inv = (iq < len && l_run > 0.f) ? a.keep_scale / l_run : 0.f;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            // a padded query's accumulator is finite but arbitrary: its context is zero by value, not by 0 * x
            const f4 o = (iq < len) ? O[mt] : (f4){0.f, 0.f, 0.f, 0.f};
            fa_store_head4(orow, mt, q4, dk, o, inv);
        }
    }
}

}  // namespace

extern "C" int ia_relpos_attention_local_supported(int T, int dk, int window) {
    return (window >= 1 && ia_relpos_attention_flash_supported(T, dk)) ? 1 : 0;
}

extern "C" int ia_relpos_attention_local(const void* qkv, const void* pos_proj, const float* bias_u, const float* bias_v,
                                         const int64_t* lens, int B, int T, int H, int dk, int window, float dropout_p,
                                         unsigned seed, void* ctx, ia_stream_t stream) {
    return ia_relpos_attention_local_lse(qkv, pos_proj, bias_u, bias_v, lens, B, T, H, dk, window, dropout_p, seed, ctx, nullptr, stream);
}

extern "C" int ia_relpos_attention_local_lse(const void* qkv, const void* pos_proj, const float* bias_u, const float* bias_v,
                                             const int64_t* lens, int B, int T, int H, int dk, int window, float dropout_p,
                                             unsigned seed, void* ctx, float* lse, ia_stream_t stream) {
    if (!qkv || !pos_proj || !bias_u || !bias_v || !lens || !ctx || B <= 0 || T <= 0 || H <= 0 || window <= 0) return IA_INVALID_VALUE;
    if (!ia_relpos_attention_local_supported(T, dk, window)) return IA_UNSUPPORTED;
    if (dropout_p < 0.f || dropout_p >= 1.f) return IA_INVALID_VALUE;
    if (!ia_is_aligned(qkv, 16) || !ia_is_aligned(pos_proj, 16) || !ia_is_aligned(ctx, 8)) return IA_INVALID_VALUE;
    // a window beyond T - 1 admits no further key: the same band with w' = T - 1 and the table advanced by w - w' rows
    const int w = window < T - 1 ? window : T - 1;
    FlArgs a;
    a.qkv = (const __bf16*)qkv; a.pl = (const __bf16*)pos_proj + (size_t)(window - w) * ((size_t)H * dk);
    a.bias_u = bias_u; a.bias_v = bias_v; a.lens = lens; a.lse = lse;
    a.ctx = (__bf16*)ctx; a.B = B; a.T = T; a.H = H; a.dk = dk; a.w = w; a.scale = 1.f / sqrtf((float)dk); a.seed = seed;
    const ia_dropout_t drop = ia_dropout_rule(dropout_p);
    a.thr = drop.thr; a.keep_scale = drop.keep_scale;
    const int nqt = (T + 63) / 64;
    const int grid = 8 * ((B * H + 7) / 8) * nqt;
    hipStream_t st = (hipStream_t)stream;
    return fa_launch<FlArgs, relpos_local_fwd_kernel<true>, relpos_local_fwd_kernel<false>>(dk == 64 && (H * dk) % 8 == 0, grid, FL_LDS,
                                                                                            st, a);
}
