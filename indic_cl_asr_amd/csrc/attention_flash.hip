// Relative-position multi-head self-attention forward, key-tile loop with online softmax (gfx950), full, local or limited-context
// by its Span.
//
//   ctx[b,i,h,:] = sum_j softmax_j( ((q_i+u_h).k_j + (q_i+v_h).p_h[centre-i+j]) / sqrt(dk) ) v_j ,   j < len_b  (and |i-j| <= w)
//
// Full span: RelPositionMultiHeadAttention.forward A/parts/submodules/multi_head_attention.py:197-250: rel_shift (:184-195) as
// index arithmetic, centre = T - 1, the [B,T,T] mask replaced by lengths (keys >= len excluded = "-10000 then zero", :108-111;
// padded queries give zero context), attention dropout on the probabilities.
// Local span: RelPositionMultiHeadAttentionLongformer.forward (:253-470) with LocalAttRelPositionalEncoding (:982-1026) for a
// symmetric window [w, w] and no global tokens: the sliding-chunk matmuls and their diagonal bookkeeping are the band
// |i - j| <= w, the position table's row r holds relative position w - r (2w + 1 rows, centre = w).  Asymmetric windows are not
// offered: the reference adds their position term to the wrong columns.  The host reduces a window beyond T - 1 to w' = T - 1
// by advancing the table pointer (row r of the 2w+1 table is row r - (w - w') of the 2w'+1 one), so the kernel's index
// arithmetic never sees a window larger than T; a window >= T - 1 gives the full span's values.
// Context span: the full span's formula and table under the attention mask of ConformerEncoder._create_masks
// (A/modules/conformer_encoder.py:686-740) for att_context_style 'regular' / 'chunked_limited': one interval of keys per query
// (attention_flash.h, FaContextSpan); the host reduces (style, left, right) to bounded integers and runs the full span when the
// context admits every pair.
//
// The kernel walks 64-key tiles (the span's: all below len, the 1 + 2 ceil(w / 64) at the most that meet the window, or those
// that meet the context's interval) and
// keeps only the running maximum, sum and output of a 16-query strip in registers, so T is unbounded (30 s audio: T' = 751);
// the head dim is any multiple of 4 up to 64 (d = 144 / 4 heads = 36: tiles zero-padded to 64 in LDS).
//
// Workgroup = (utterance, head, 64 queries), 4 waves x 16 queries.  Per 64-key tile, staged once per workgroup in LDS
// (K, V row-major [key][dk], 128 position rows covering the four waves' bands; 16-byte slots XOR-swizzled by row & 7):
//   R^T = P_band (q+v)^T   [80 positions x 16 queries]   10 x v_mfma_f32_16x16x32_bf16    (A = position rows from LDS)
//   S^T = K (q+u)^T        [64 keys x 16 queries]          8 MFMAs
//   the skew bd[i][j] = R[i][j - j0 + 15 - il] goes through a wave-private bf16 strip written at column rr + il + 1, so
//   that the reads are aligned 8-byte vectors; scores / softmax live in the TRANSPOSED accumulators: a lane owns one
//   query (column) and 16 keys (registers), the row maximum / sum are in-lane plus two cross-lane steps, and the
//   probabilities ARE the B operand of
//   O^T += V^T P^T         [64 dv x 16 queries]             8 MFMAs   (A = V^T fragments by ds_read_b64_tr_b16 from the
//   row-major V tile: no pre-transposed V copy, no probability round trip through LDS).
// The optional lse (natural-log log-sum-exp per query, 0 for padded queries) is what the backward recomputes P from.
#include <type_traits>

#include "attention_flash.h"

namespace {

constexpr int FA_KT = 64;                  // keys per tile
constexpr int FA_STAGE = 2 * FA_T64 + FA_PBUF;    // K | V | P = 32 KB per stage
constexpr int FA_SR_BYTES = 16 * FA_SR_LD * 2;
constexpr int FA_LDS = FA_STAGE + 4 * FA_SR_BYTES;       // 46 080 B: three workgroups per CU

struct FaArgs {
    const __bf16* qkv; const __bf16* pl; const float* bias_u; const float* bias_v; const int64_t* lens;
    __bf16* ctx; int B, T, H, dk; float scale; unsigned seed, thr; float keep_scale;
    float* lse;   // optional [B*H, T]: log-sum-exp of each query's scaled scores (the backward recomputes P = exp(s - lse))
    FaSpanArgs sp;   // the span's integers (local: w, 0 <= w <= T - 1).  Last: the full span does not read them
};

template <bool DK64, class Span>
__global__ __launch_bounds__(FA_THREADS, 3) void relpos_flash_fwd_kernel(FaArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, q4 = lane >> 4;
    const int T = a.T, H = a.H, dk = a.dk, d = H * dk;
    const Span span(T, a.sp);
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
    unsigned char* sR = smem + FA_STAGE + wave * FA_SR_BYTES;

    // ---- B fragments (q+u)^T and (q+v)^T: lane (query c, q4) holds dk elements 32 ks + 8 q4 .. +7 of its query
    bf8 Qu[2], Qv[2];
    {
        const int iqc = iq < T ? iq : T - 1;
        const __bf16* qrow = a.qkv + ((size_t)b * T + iqc) * (3 * d) + h * dk;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) fa_query_frags<DK64>(qrow, a.bias_u, a.bias_v, h, dk, ks, q4, Qu[ks], Qv[ks]);
    }

    // ---- staging (FaKvpStage): tile t + 1 -> registers (8 x 16 B per thread) while tile t is computed from the ONE LDS stage,
    // then barrier, registers -> LDS, barrier.  One stage (45 KB with the strips) keeps three workgroups on a CU: the 768
    // workgroups of a 32 x 376-frame batch are all resident (two stages = 512 slots = a second, half-empty round: 41 us;
    // measured per-workgroup cost 5 us + 3.3 us per key tile), and three waves per SIMD hide each other's LDS round trips.
    FaKvpStage<DK64> stage(a.qkv, a.pl, smem, b, h, T, d, dk, I0, span.centre(), tid);

    const FaTiles ktiles = span.tiles(FaQueryOwner{}, I0, len);   // the key tiles of this query tile
    stage.fetch(ktiles.lo);
    stage.commit();
    __syncthreads();

    f4 O[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) O[mt] = (f4){0.f, 0.f, 0.f, 0.f};
    float m_run = IA_NEG_INF, l_run = 0.f;      // running maximum of this lane's query, this lane's share of the sum
    const float scale2 = a.scale * 1.44269504088896341f;

    for (int t = ktiles.lo; t < ktiles.end; ++t) {
        const unsigned char* sK = smem;
        const unsigned char* sV = sK + FA_T64;
        const unsigned char* sP = sK + 2 * FA_T64;
        if (t + 1 < ktiles.end) stage.fetch(t + 1);
        const int j0 = t * FA_KT;
        // ---- band R^T: rows = positions 16 (3 - wave + rt) + 4 q4 + r of the staged 128, columns = queries -> strip
        fa_band_to_strip(sP, sR, (3 - wave) * 16, Qv, c, q4);
        // ---- S^T = K (q+u)^T
        f4 S[4];
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
            S[jt] = (f4){0.f, 0.f, 0.f, 0.f};
            const int row = jt * 16 + c;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
                S[jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa_frag(sK, row, ks, q4), Qu[ks], S[jt], 0, 0, 0);
        }
        // ---- scores: lane (query c, q4), key j = j0 + 16 jt + 4 q4 + r; band element at strip column 16 jt + 4 q4 + r + 16
        // scores in base-2 units (scale * log2 e folded into one multiply, exp2 directly: no multiply per exponential); the
        // mask only exists in the tiles that straddle the length or the window's edge (uniform branch)
        float tmax = IA_NEG_INF;
        if (span.tile_unmasked(j0, iw, len)) {
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
            const auto admitted = span.admit(FaQueryOwner{}, iq, true, len);   // this query's keys
#pragma unroll
            for (int jt = 0; jt < 4; ++jt) {
                union { uint2 u; __bf16 e[4]; } bd;
                bd.u = *reinterpret_cast<const uint2*>(sR + (c * FA_SR_LD + jt * 16 + q4 * 4 + 16) * 2);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = j0 + jt * 16 + q4 * 4 + r;
                    const float s = admitted(j) ? (S[jt][r] + (float)bd.e[r]) * scale2 : IA_NEG_INF;
                    S[jt][r] = s;
                    tmax = fmaxf(tmax, s);
                }
            }
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float m_new = fmaxf(m_run, tmax);
        // the exponentials' reference: the new maximum; 0 while a sparse span has shown this query no key (-inf - -inf = NaN)
        float m_ref = m_new;
        if constexpr (Span::kSparseTiles) m_ref = (m_new == IA_NEG_INF) ? 0.f : m_new;
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_ref);   // exp2(-inf) = 0 on the first tile
        m_run = m_new;
        float psum = 0.f;
        bf8 Pf[2];
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
            unsigned rnd4 = 0;
            if (a.thr > 0) rnd4 = fa_keep_rand4(a.seed, bh, T, iq, (j0 + jt * 16 + q4 * 4) >> 2);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float p = __builtin_amdgcn_exp2f(S[jt][r] - m_ref);   // exp2(-inf) = 0 for excluded keys
                psum += p;
                // (the keep scale 1/(1-p) of the dropout is applied once, to the normalised output)
                if (a.thr > 0) p = (((rnd4 >> (8 * r)) & 0xFFu) >= a.thr) ? p : 0.f;
                Pf[jt >> 1][(jt & 1) * 4 + r] = (__bf16)p;
            }
        }
        l_run = l_run * alpha + psum;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) O[mt][r] *= alpha;
        // ---- O^T += V^T P^T: k-step kk covers keys 32 kk .. +31 in the order (16-key tile 2kk: 4 q4 + e, tile 2kk+1: 4 q4 + e)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                // 16-lane group q4 reads the 4-key x 16-dv blocks (keys 32 kk + 4 q4 + 0..3 and + 16); lane 4 qq + p of the group
                // supplies row qq, dv 16 mt + 4 p .. + 3
                const int qq = c >> 2, p = c & 3;
                const int rowA = kk * 32 + q4 * 4 + qq;
                const bf8 vf = fa_tr_pair(sV, rowA, rowA + 16, mt * 2 + (p >> 1), p & 1);
                O[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, Pf[kk], O[mt], 0, 0, 0);
            }
        __syncthreads();                      // every wave is done with the stage
        if (t + 1 < ktiles.end) {
            stage.commit();
            __syncthreads();
        }
    }
    // ---- normalise and store: lane (query c, q4) holds dv = 16 mt + 4 q4 + r
    l_run += __shfl_xor(l_run, 16, 64);
    l_run += __shfl_xor(l_run, 32, 64);
    if (iq < T) {
        // natural-log LSE for the backward: (m + log2 l) ln 2
        if (a.lse && q4 == 0) a.lse[(size_t)bh * T + iq] = (iq < len && l_run > 0.f) ? (m_run + __builtin_amdgcn_logf(l_run)) * 0.69314718055994531f : 0.f;
        const float inv = (iq < len && l_run > 0.f) ? a.keep_scale / l_run : 0.f;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            f4 o = O[mt];
            // under a sparse span a padded query's accumulator is finite but arbitrary: zero by value, not by 0 * x
            if constexpr (Span::kSparseTiles) o = (iq < len) ? O[mt] : (f4){0.f, 0.f, 0.f, 0.f};
            fa_store_head4(orow, mt, q4, dk, o, inv);
        }
    }
}

// host: the forward under one span, after the entry point's argument checks
template <class Span>
int fa_forward(const void* qkv, const __bf16* pl, const float* bias_u, const float* bias_v, const int64_t* lens, int B, int T, int H,
               int dk, FaSpanArgs sp, float dropout_p, unsigned seed, void* ctx, float* lse, ia_stream_t stream) {
    FaArgs a;
    a.qkv = (const __bf16*)qkv; a.pl = pl; a.bias_u = bias_u; a.bias_v = bias_v; a.lens = lens;
    a.lse = lse;
    a.ctx = (__bf16*)ctx; a.B = B; a.T = T; a.H = H; a.dk = dk; a.sp = sp; a.scale = 1.f / sqrtf((float)dk); a.seed = seed;
    const ia_dropout_t drop = ia_dropout_rule(dropout_p);
    a.thr = drop.thr; a.keep_scale = drop.keep_scale;
    const int nqt = (T + 63) / 64;
    const int grid = 8 * ((B * H + 7) / 8) * nqt;
    return fa_launch<FaArgs, relpos_flash_fwd_kernel<true, Span>, relpos_flash_fwd_kernel<false, Span>>(
        dk == 64 && (H * dk) % 8 == 0, grid, FA_LDS, (hipStream_t)stream, a);
}

}  // namespace

extern "C" int ia_relpos_attention_flash_supported(int T, int dk) { return (T > 0 && dk > 0 && dk <= 64 && dk % 4 == 0) ? 1 : 0; }

extern "C" int ia_relpos_attention_flash(const void* qkv, const void* pos_proj, const float* bias_u, const float* bias_v,
                                         const int64_t* lens, int B, int T, int H, int dk, float dropout_p, unsigned seed,
                                         void* ctx, ia_stream_t stream) {
    return ia_relpos_attention_flash_lse(qkv, pos_proj, bias_u, bias_v, lens, B, T, H, dk, dropout_p, seed, ctx, nullptr, stream);
}

extern "C" int ia_relpos_attention_flash_lse(const void* qkv, const void* pos_proj, const float* bias_u, const float* bias_v,
                                             const int64_t* lens, int B, int T, int H, int dk, float dropout_p, unsigned seed,
                                             void* ctx, float* lse, ia_stream_t stream) {
    if (!qkv || !pos_proj || !bias_u || !bias_v || !lens || !ctx || B <= 0 || T <= 0 || H <= 0) return IA_INVALID_VALUE;
    if (!ia_relpos_attention_flash_supported(T, dk)) return IA_UNSUPPORTED;
    if (dropout_p < 0.f || dropout_p >= 1.f) return IA_INVALID_VALUE;
    if (!ia_is_aligned(qkv, 16) || !ia_is_aligned(pos_proj, 16) || !ia_is_aligned(ctx, 8)) return IA_INVALID_VALUE;
    return fa_forward<FaFullSpan>(qkv, (const __bf16*)pos_proj, bias_u, bias_v, lens, B, T, H, dk, FaSpanArgs{T - 1, 0, 0}, dropout_p, seed, ctx, lse, stream);
}

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
    return fa_forward<FaLocalSpan>(qkv, (const __bf16*)pos_proj + (size_t)(window - w) * ((size_t)H * dk), bias_u, bias_v, lens, B, T, H,
                                   dk, FaSpanArgs{w, 0, 0}, dropout_p, seed, ctx, lse, stream);
}

// ---- limited context: (style, left, right) -> the context span's bounded integers (attention_flash.h), or "admits every pair"
extern "C" int ia_relpos_attention_context_supported(int T, int dk, int style, int left, int right) {
    FaSpanArgs sp;
    return (fa_context_args(T, style, left, right, &sp) != FA_CTX_INVALID && ia_relpos_attention_flash_supported(T, dk)) ? 1 : 0;
}

extern "C" int ia_relpos_attention_context(const void* qkv, const void* pos_proj, const float* bias_u, const float* bias_v,
                                           const int64_t* lens, int B, int T, int H, int dk, int style, int left, int right,
                                           float dropout_p, unsigned seed, void* ctx, ia_stream_t stream) {
    return ia_relpos_attention_context_lse(qkv, pos_proj, bias_u, bias_v, lens, B, T, H, dk, style, left, right, dropout_p, seed, ctx,
                                           nullptr, stream);
}

extern "C" int ia_relpos_attention_context_lse(const void* qkv, const void* pos_proj, const float* bias_u, const float* bias_v,
                                               const int64_t* lens, int B, int T, int H, int dk, int style, int left, int right,
                                               float dropout_p, unsigned seed, void* ctx, float* lse, ia_stream_t stream) {
    if (!qkv || !pos_proj || !bias_u || !bias_v || !lens || !ctx || B <= 0 || T <= 0 || H <= 0) return IA_INVALID_VALUE;
    FaSpanArgs sp;
    const int kind = fa_context_args(T, style, left, right, &sp);
    if (kind == FA_CTX_INVALID) return IA_INVALID_VALUE;
    if (!ia_relpos_attention_flash_supported(T, dk)) return IA_UNSUPPORTED;
    if (dropout_p < 0.f || dropout_p >= 1.f) return IA_INVALID_VALUE;
    if (!ia_is_aligned(qkv, 16) || !ia_is_aligned(pos_proj, 16) || !ia_is_aligned(ctx, 8)) return IA_INVALID_VALUE;
    if (kind == FA_CTX_FULL)   // every pair admitted: the full span's kernel and bits
        return fa_forward<FaFullSpan>(qkv, (const __bf16*)pos_proj, bias_u, bias_v, lens, B, T, H, dk, FaSpanArgs{T - 1, 0, 0}, dropout_p, seed,
                                      ctx, lse, stream);
    return fa_forward<FaContextSpan>(qkv, (const __bf16*)pos_proj, bias_u, bias_v, lens, B, T, H, dk, sp, dropout_p, seed, ctx, lse, stream);
}
