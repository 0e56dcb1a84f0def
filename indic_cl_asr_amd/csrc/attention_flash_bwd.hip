// Relative-position multi-head self-attention BACKWARD, key-tiled (gfx950), full, local or limited-context by its Span (the
// context span: the full span's centre, table and dBand layout, the pairs and tiles of FaContextSpan): no [T,T] probability /
// score-gradient matrices in HBM, any T, head dim any multiple of 4 up to 64.  Autograd of RelPositionMultiHeadAttention.forward
// (A/parts/submodules/multi_head_attention.py:197-250; local span: of the band |i - j| <= w of
// RelPositionMultiHeadAttentionLongformer.forward) with the forward of attention_flash.hip (same span and tile ranges, same
// dropout hash, the forward's per-query log-sum-exp).  c = the span's centre, T - 1 or w:
//
//   s_ij = ((q_i+u).k_j + (q_i+v).p[c-i+j]) / sqrt(dk),  admissible iff j < len, i < len (and |i-j| <= w)
//   P = exp(s - lse_i) on admissible pairs, else 0 (by value: a clamped position row gives a finite score that means nothing)
//   Pd = dropout(P),  dP = keep o (dO V^T),  D_i = dO_i . O_i,  dS = P o (dP - D) / sqrt(dk)
//   d(q+u) = dS K     d(q+v)_i = sum_j dS_ij p[c-i+j]     dK = dS^T (q+u)     dV = Pd^T dO
//   dp[r] = sum_{b,i} dS_{i, r-c+i} (q_i+v)      dq = d(q+u) + d(q+v)     du = sum d(q+u)    dv = sum d(q+v)
//
// Two kernels, each owning its outputs exclusively (no atomics, bit-reproducible):
//   relpos_flash_bwd_q_kernel   workgroup = (utterance, head, 64 queries), 4 waves x 16 queries, walks the key tiles like
//       the forward (transposed accumulators: lane = query).  Recomputes R^T, S^T, P; dP^T = V dO^T; dS.  dS is the B
//       operand of d(q+u)^T += K^T dS^T as it lies in the accumulators, and goes through a wave-private band strip
//       [query][band row] for d(q+v)^T += P_band^T dS_band^T (band row rr = j - j0 + 15 - il: the inverse of the forward's
//       skew).  The same strip, tile by tile, is the band-skewed dS on the relative-position axis
//       dBand[h][b*T+i][pad0 + c-i+j] that the position-projection gradient dp = dBand^T (q+v) contracts as a plain TN GEMM
//       (csrc/gemm_tn.hip) -- the one matrix that still goes through HBM, [T, ~2T] under the full span and [T, ~2w] under the
//       local one.  Strip column s of (wave iw, tile j0) is relative position c - iw - 15 + j0 + s on an UNCLAMPED axis:
//       consecutive tiles continue each other's columns (64 per tile, the last 16 carried into the next tile's flush), so every
//       dBand element of a query row has one writer; what no (wave, tile) writes is the memset's zero.
//   relpos_flash_bwd_kv_kernel  workgroup = (utterance, head, 64 keys), 4 waves x 16 keys (lane = key), walks the query
//       tiles.  S = (Q+u) K^T and the band (q+v) p^T in the key-major orientation (two 16x16 position tiles per 16
//       queries, re-indexed through a wave-private strip), P, dP, then dV^T += dO^T Pd and dK^T += (Q+u)^T dS with the
//       probabilities / score gradients used as B operands straight from the accumulators and the A operands read from
//       the row-major query tiles with ds_read_b64_tr_b16.
// LDS tiles: 128-byte rows (64 bf16, zero-padded beyond dk), 16-byte slots XOR-swizzled by row & 7, one stage + register
// prefetch of the next tile (two workgroups per CU hide the two barriers per tile).  The query-owner uses the forward's
// K | V | P stage as it is, the key-owner builds its Qu | Qv | dO | P | lse, D stage from the same fetch / commit pair.
#include "attention_flash.h"
#include "partials.h"

namespace {

struct FbArgs {
    const __bf16* qkv; const __bf16* pl; const float* bias_u; const float* bias_v; const int64_t* lens;
    const __bf16* ctx; const __bf16* dctx; const float* lse;
    __bf16* dqkv; __bf16* dBand; __bf16* QvHM; float* D; float* part;
    int B, T, H, dk, w, Rs, pad0; float scale; unsigned seed, thr; float keep_scale;   // w: the local span's, 0 <= w <= T - 1
    int w2, chunk;   // with w the context span's integers (FaSpanArgs).  Last: the other spans do not read them
};

// a 16-byte chunk at dBand column gcol is written: inside [0, rs) of a bounded band, right of column 0 of an unbounded one
template <class Span>
__device__ __forceinline__ bool fb_chunk_in_row(int gcol, int rs) {
    if constexpr (Span::kBoundedBand) return gcol >= 0 && gcol + 8 <= rs;
    else return gcol >= 0;
}

// ======================================================================================================== query-owner
template <bool DK64, class Span>
__global__ __launch_bounds__(FA_THREADS, 2) void relpos_flash_bwd_q_kernel(FbArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, q4 = lane >> 4;
    const int T = a.T, H = a.H, dk = a.dk, d = H * dk, B = a.B;
    const Span span(T, FaSpanArgs{a.w, a.w2, a.chunk});
    const int nqt = (T + 63) / 64;
    const FaWg wg = fa_wg(B, T, H, a.lens);
    if (wg.len < 0) return;
    const int bh = wg.bh, qt = wg.tile, h = wg.h, b = wg.b, len = wg.len;
    const int I0 = qt * 64, iw = I0 + wave * 16, iq = iw + c;
    const int iqc = iq < T ? iq : T - 1;
    const bool qvalid = iq < len;
    float* part_row = a.part + (size_t)(b * nqt + qt) * (2 * d);

    // ---- this lane's query: (q+u), (q+v), dO as MFMA B fragments (dk elements 32 ks + 8 q4 .. +7), D = dO . O
    bf8 Qu[2], Qv[2], dOa[2];
    float Drow = 0.f;
    {
        const __bf16* qrow = a.qkv + ((size_t)b * T + iqc) * (3 * d) + h * dk;
        const __bf16* orow = a.ctx + ((size_t)b * T + iqc) * d + h * dk;
        const __bf16* grow = a.dctx + ((size_t)b * T + iqc) * d + h * dk;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            union { uint4 u; __bf16 e[8]; bf8 v; } o, g;
            fa_query_frags<DK64>(qrow, a.bias_u, a.bias_v, h, dk, ks, q4, Qu[ks], Qv[ks]);
            o.u = fa_load_slot<DK64>(orow, ks * 4 + q4, dk);
            g.u = fa_load_slot<DK64>(grow, ks * 4 + q4, dk);
            dOa[ks] = g.v;
#pragma unroll
            for (int j = 0; j < 8; ++j) Drow += (float)g.e[j] * (float)o.e[j];
            if (iq < T)   // head-major copy of (q+v): the X operand of dp = dBand^T (q+v)
                *reinterpret_cast<bf8*>(a.QvHM + ((size_t)(h * B + b) * T + iq) * 64 + ks * 32 + q4 * 8) = Qv[ks];
        }
        Drow += __shfl_xor(Drow, 16, 64);
        Drow += __shfl_xor(Drow, 32, 64);
        if (!qvalid) Drow = 0.f;
        if (iq < T && q4 == 0) a.D[(size_t)bh * T + iq] = Drow;
    }
    const float lse_i = qvalid ? a.lse[(size_t)bh * T + iq] : 0.f;
    __bf16* dqrow = a.dqkv + ((size_t)b * T + iqc) * (3 * d) + h * dk;
    if (I0 >= len) {   // workgroup-uniform: padded queries only -- zero gradient rows, zero bias partials
        if (iq < T)
            for (int mt = 0; mt < 4; ++mt) fa_store_head4(dqrow, mt, q4, dk, (f4){0.f, 0.f, 0.f, 0.f});
        if (tid < 2 * dk) part_row[(tid / dk) * d + h * dk + (tid % dk)] = 0.f;
        return;
    }
    const unsigned char* sK = smem;
    const unsigned char* sV = smem + FA_T64;
    const unsigned char* sP = smem + 2 * FA_T64;
    unsigned char* sR = smem + 2 * FA_T64 + FA_PBUF + wave * FB_Q_STRIP;     // forward band strip [16][104] bf16
    unsigned char* sB = sR + 16 * FA_SR_LD * 2;                               // dS band strip      [16][120] bf16
    for (int i = lane; i < 16 * FB_SB_LD * 2 / 16; i += 64) reinterpret_cast<uint4*>(sB)[i] = make_uint4(0, 0, 0, 0);

    FaKvpStage<DK64> stage(a.qkv, a.pl, smem, b, h, T, d, dk, I0, span.centre(), tid);

    const FaTiles ktiles = span.tiles(FaQueryOwner{}, I0, len);                  // the key tiles of this query tile, as the forward walks them
    const auto admitted = span.admit(FaQueryOwner{}, iq, qvalid, len);       // this query's keys
    stage.fetch(ktiles.lo);
    stage.commit();
    __syncthreads();

    f4 dQu[4], dQv[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) { dQu[mt] = (f4){0.f, 0.f, 0.f, 0.f}; dQv[mt] = (f4){0.f, 0.f, 0.f, 0.f}; }
    // band flush: lane -> (row, two 16-byte chunks) of the wave's [16][64] slab; global row of query iw + row
    const int frow = lane >> 2, fch = (lane & 3) * 2;
    __bf16* brow = a.dBand + ((size_t)(h * B + b) * T + (iw + frow < T ? iw + frow : T - 1)) * a.Rs;
    const bool fvalid = iw + frow < T;
    const int pw0 = (3 - wave) * 16;   // first staged position row of this wave's band

    for (int t = ktiles.lo; t < ktiles.end; ++t) {
        if (t + 1 < ktiles.end) stage.fetch(t + 1);
        const int j0 = t * 64;
        // ---- R^T (band) -> forward strip
        fa_band_to_strip(sP, sR, pw0, Qv, c, q4);
        // ---- S^T = K (q+u)^T ,  dP^T = V dO^T
        f4 S[4], dP[4];
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
            S[jt] = (f4){0.f, 0.f, 0.f, 0.f};
            dP[jt] = (f4){0.f, 0.f, 0.f, 0.f};
            const int row = jt * 16 + c;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                S[jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa_frag(sK, row, ks, q4), Qu[ks], S[jt], 0, 0, 0);
                dP[jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa_frag(sV, row, ks, q4), dOa[ks], dP[jt], 0, 0, 0);
            }
        }
        fb_lds_fence();
        // ---- P, dS: lane (query c, q4), key j = j0 + 16 jt + 4 q4 + r
        bf8 dSf[2];
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
            union { uint2 u; __bf16 e[4]; } bd;
            bd.u = *reinterpret_cast<const uint2*>(sR + (c * FA_SR_LD + jt * 16 + q4 * 4 + 16) * 2);
            unsigned rnd4 = 0;
            if (a.thr > 0) rnd4 = fa_keep_rand4(a.seed, bh, T, iq, (j0 + jt * 16 + q4 * 4) >> 2);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = j0 + jt * 16 + q4 * 4 + r;
                const float s = (S[jt][r] + (float)bd.e[r]) * a.scale;
                const float p = admitted(j) ? __expf(s - lse_i) : 0.f;
                float g = dP[jt][r];
                if (a.thr > 0) g = (((rnd4 >> (8 * r)) & 0xFFu) >= a.thr) ? g * a.keep_scale : 0.f;
                const float ds = p * (g - Drow) * a.scale;
                const __bf16 dsb = (__bf16)ds;
                dSf[jt >> 1][(jt & 1) * 4 + r] = dsb;
                S[jt][r] = (float)dsb;   // kept for the strip
            }
        }
        // ---- d(q+u)^T += K^T dS^T
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const int qq = c >> 2, p = c & 3;
                const int rowA = kk * 32 + q4 * 4 + qq;
                const bf8 kf = fa_tr_pair(sK, rowA, rowA + 16, mt * 2 + (p >> 1), p & 1);
                dQu[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, dSf[kk], dQu[mt], 0, 0, 0);
            }
        // ---- band strip of this tile: zero the 96 band columns, then strip[c][jl + 15 - c] = dS
        for (int i = lane; i < 16 * 12; i += 64) {
            const int row = i / 12, ch = i - row * 12;
            *reinterpret_cast<uint4*>(sB + (row * FB_SB_LD + ch * 8) * 2) = make_uint4(0, 0, 0, 0);
        }
        fb_lds_fence();
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                *reinterpret_cast<__bf16*>(sB + (c * FB_SB_LD + jt * 16 + q4 * 4 + r + 15 - c) * 2) = (__bf16)S[jt][r];
        fb_lds_fence();
        // ---- d(q+v)^T += P_band^T dS_band^T : k-step kk = band rows 32 kk .. +31 (lane element e <-> row 32 kk + 8 q4 + e)
#pragma unroll
        for (int kk = 0; kk < 3; ++kk) {
            const bf8 bfrag = *reinterpret_cast<const bf8*>(sB + (c * FB_SB_LD + kk * 32 + q4 * 8) * 2);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const int qq = c >> 2, p = c & 3;
                int rowA = pw0 + kk * 32 + q4 * 8 + qq, rowB = rowA + 4;
                // band rows >= 79 are zero in the strip; so are the band rows of clamped position rows (inadmissible pairs)
                rowA = rowA < 127 ? rowA : 127; rowB = rowB < 127 ? rowB : 127;
                const bf8 pf = fa_tr_pair(sP, rowA, rowB, mt * 2 + (p >> 1), p & 1);
                dQv[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, bfrag, dQv[mt], 0, 0, 0);
            }
        }
        // ---- flush band columns [0,64) (first 16 merged with the carry of the previous tile) to dBand, keep [64,80) as carry
        {
            uint4 v0 = *reinterpret_cast<const uint4*>(sB + (frow * FB_SB_LD + fch * 8) * 2);
            uint4 v1 = *reinterpret_cast<const uint4*>(sB + (frow * FB_SB_LD + fch * 8 + 8) * 2);
            if ((lane & 3) == 0) {   // disjoint supports: one side is an explicit +0 everywhere
                const uint4 c0 = *reinterpret_cast<const uint4*>(sB + (frow * FB_SB_LD + 96) * 2);
                const uint4 c1 = *reinterpret_cast<const uint4*>(sB + (frow * FB_SB_LD + 104) * 2);
                v0.x |= c0.x; v0.y |= c0.y; v0.z |= c0.z; v0.w |= c0.w;
                v1.x |= c1.x; v1.y |= c1.y; v1.z |= c1.z; v1.w |= c1.w;
                const uint4 n0 = *reinterpret_cast<const uint4*>(sB + (frow * FB_SB_LD + 64) * 2);
                const uint4 n1 = *reinterpret_cast<const uint4*>(sB + (frow * FB_SB_LD + 72) * 2);
                *reinterpret_cast<uint4*>(sB + (frow * FB_SB_LD + 96) * 2) = n0;
                *reinterpret_cast<uint4*>(sB + (frow * FB_SB_LD + 104) * 2) = n1;
            }
            // gcol (and a bounded band's Rs) are multiples of 8: a 16-byte chunk lies inside the dBand row or outside it, and
            // outside it every value is an inadmissible pair's zero.  Unbounded band: gcol is negative only in a partial last
            // wave (T - iw < 16), whose leading band columns are all zero
            if (fvalid) {
                const int gcol = span.centre() - 15 - iw + j0 + a.pad0 + fch * 8;
                if (fb_chunk_in_row<Span>(gcol, a.Rs)) *reinterpret_cast<uint4*>(brow + gcol) = v0;
                if (fb_chunk_in_row<Span>(gcol + 8, a.Rs)) *reinterpret_cast<uint4*>(brow + gcol + 8) = v1;
            }
        }
        __syncthreads();
        if (t + 1 < ktiles.end) {
            stage.commit();
            __syncthreads();
        }
    }
    // ---- last carry -> dBand columns 64 .. 79 behind the last processed tile
    fb_lds_fence();
    if ((lane & 3) == 0 && fvalid) {
        const int gcol = span.centre() - 15 - iw + (ktiles.end - 1) * 64 + a.pad0 + 64;
        const uint4 c0 = *reinterpret_cast<const uint4*>(sB + (frow * FB_SB_LD + 96) * 2);
        const uint4 c1 = *reinterpret_cast<const uint4*>(sB + (frow * FB_SB_LD + 104) * 2);
        if (!Span::kBoundedBand || fb_chunk_in_row<Span>(gcol, a.Rs)) *reinterpret_cast<uint4*>(brow + gcol) = c0;
        if (!Span::kBoundedBand || fb_chunk_in_row<Span>(gcol + 8, a.Rs)) *reinterpret_cast<uint4*>(brow + gcol + 8) = c1;
    }
    // ---- dq = d(q+u) + d(q+v): lane (query c, q4) holds e = 16 mt + 4 q4 + r
    if (iq < T) {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) fa_store_head4(dqrow, mt, q4, dk, dQu[mt] + dQv[mt]);
    }
    // ---- bias gradients: sums over the workgroup's 64 queries -> this workgroup's slice of its partial row
    float* red = reinterpret_cast<float*>(smem);   // [4 waves][2][64] (the K tile is no longer read: barrier above)
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float su = dQu[mt][r], sv = dQv[mt][r];
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) { su += __shfl_xor(su, o, 64); sv += __shfl_xor(sv, o, 64); }
            if (c == 0) {
                red[(wave * 2 + 0) * 64 + mt * 16 + q4 * 4 + r] = su;
                red[(wave * 2 + 1) * 64 + mt * 16 + q4 * 4 + r] = sv;
            }
        }
    __syncthreads();
    if (tid < 2 * dk) {
        const int which = tid / dk, e = tid % dk;
        part_row[which * d + h * dk + e] = (red[(0 * 2 + which) * 64 + e] + red[(1 * 2 + which) * 64 + e]) +
                                           (red[(2 * 2 + which) * 64 + e] + red[(3 * 2 + which) * 64 + e]);
    }
}

// ========================================================================================================== key-owner
template <bool DK64, class Span>
__global__ __launch_bounds__(FA_THREADS, 2) void relpos_flash_bwd_kv_kernel(FbArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, q4 = lane >> 4;
    const int T = a.T, H = a.H, dk = a.dk, d = H * dk, B = a.B;
    const Span span(T, FaSpanArgs{a.w, a.w2, a.chunk});
    const FaWg wg = fa_wg(B, T, H, a.lens);
    if (wg.len < 0) return;
    const int bh = wg.bh, kt = wg.tile, h = wg.h, b = wg.b, len = wg.len;
    const int J0 = kt * 64, jw = J0 + wave * 16, j = jw + c;
    const int jc = j < T ? j : T - 1;
    const bool kvalid = j < len;
    __bf16* dkrow = a.dqkv + ((size_t)b * T + jc) * (3 * d) + d + h * dk;
    __bf16* dvrow = dkrow + d;
    if (J0 >= len) {   // workgroup-uniform: padded keys only
        if (j < T)
            for (int mt = 0; mt < 4; ++mt) {
                fa_store_head4(dkrow, mt, q4, dk, (f4){0.f, 0.f, 0.f, 0.f});
                fa_store_head4(dvrow, mt, q4, dk, (f4){0.f, 0.f, 0.f, 0.f});
            }
        return;
    }
    // ---- this lane's key: K and V rows as MFMA B fragments
    bf8 Kf[2], Vf[2];
    {
        const __bf16* krow = a.qkv + ((size_t)b * T + jc) * (3 * d) + d + h * dk;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            union { uint4 u; bf8 v; } k, v;
            k.u = fa_load_slot<DK64>(krow, ks * 4 + q4, dk);
            v.u = fa_load_slot<DK64>(krow + d, ks * 4 + q4, dk);
            Kf[ks] = k.v; Vf[ks] = v.v;
        }
    }
    const unsigned char* sQu = smem;
    const unsigned char* sQv = smem + FA_T64;
    const unsigned char* sdO = smem + 2 * FA_T64;
    const unsigned char* sP = smem + 3 * FA_T64;
    const float* sL = reinterpret_cast<const float*>(smem + 3 * FA_T64 + FA_PBUF);   // lse[64] | D[64]
    unsigned char* s3 = smem + FB_KV_STAGE + wave * (16 * FB_S3_LD * 2);

    // staging: thread -> slot sl = tid & 7 of rows (tid >> 3) and (tid >> 3) + 32; the biases of its 8 elements in registers
    float bu[8], bv[8];
    {
        const int sl = tid & 7;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int ee = sl * 8 + e;
            bu[e] = (ee < dk) ? a.bias_u[h * dk + ee] : 0.f;
            bv[e] = (ee < dk) ? a.bias_v[h * dk + ee] : 0.f;
        }
    }
    uint4 rq[2], rg[2], rp[4];
    float rl = 0.f;
    const __bf16* qbase = a.qkv + (size_t)b * T * (3 * d) + h * dk;
    const __bf16* gbase = a.dctx + (size_t)b * T * d + h * dk;
    const __bf16* pbase = a.pl + h * dk;
    const int centre = span.centre();
    const auto fetch = [&](int t) {   // position rows centre - i0 - 63 + J0 .. + 127 clamped to [0, 2 centre]
        const int i0 = t * 64;
        fa_fetch_rows<DK64, false>(rq, qbase, 3 * d, i0, T - 1, dk, tid);
        fa_fetch_rows<DK64, false>(rg, gbase, d, i0, T - 1, dk, tid);
        fa_fetch_rows<DK64, true>(rp, pbase, d, centre - i0 - 63 + J0, 2 * centre, dk, tid);
        if (tid < 128) {
            int q = i0 + (tid & 63); q = q < T ? q : T - 1;
            rl = (tid < 64 ? a.lse : a.D)[(size_t)bh * T + q];
        }
    };
    const auto commit = [&]() {   // (q+u) and (q+v) are made here, from the fetched q rows and the thread's biases
        uint4 ru[2], rw[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            union { uint4 u; __bf16 e[8]; } q, u, v;
            q.u = rq[i];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                u.e[e] = (__bf16)((float)q.e[e] + bu[e]);
                v.e[e] = (__bf16)((float)q.e[e] + bv[e]);
            }
            ru[i] = u.u; rw[i] = v.u;
        }
        fa_commit_rows(smem, ru, tid);
        fa_commit_rows(smem + FA_T64, rw, tid);
        fa_commit_rows(smem + 2 * FA_T64, rg, tid);
        fa_commit_rows(smem + 3 * FA_T64, rp, tid);
        if (tid < 128) reinterpret_cast<float*>(smem + 3 * FA_T64 + FA_PBUF)[tid] = rl;
    };

    const FaTiles qtiles = span.tiles(FaKeyOwner{}, J0, len);                 // the query tiles of this key tile
    const auto admitted = span.admit(FaKeyOwner{}, j, kvalid, len);       // this key's queries
    fetch(qtiles.lo);
    commit();
    __syncthreads();

    f4 dK[4], dV[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) { dK[mt] = (f4){0.f, 0.f, 0.f, 0.f}; dV[mt] = (f4){0.f, 0.f, 0.f, 0.f}; }

    for (int t = qtiles.lo; t < qtiles.end; ++t) {
        if (t + 1 < qtiles.end) fetch(t + 1);
        const int I0 = t * 64;
        // ---- band: for the 16 queries of tile `it` the wave's keys need position rows n0 .. n0 + 31, n0 = 48 - 16 it + 16 w
        //      X_A[m][n] = (q+v)_{16 it + m} . p[n0 + n], X_B with n0 + 16;  bd[il = 16 it + m][key c] = c <= m ? X_A[m][15 - m + c]
        //      : X_B[m][c - m - 1]  ->  strip[key][il]
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            f4 XA = (f4){0.f, 0.f, 0.f, 0.f}, XB = (f4){0.f, 0.f, 0.f, 0.f};
            const int qrow = it * 16 + c;
            const int n0 = 48 - 16 * it + 16 * wave;
            const int pa = n0 + c, pb = n0 + 16 + c;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const bf8 qf = fa_frag(sQv, qrow, ks, q4), fa = fa_frag(sP, pa, ks, q4), fb = fa_frag(sP, pb, ks, q4);
                XA = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf, fa, XA, 0, 0, 0);
                XB = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf, fb, XB, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {   // lane = position column c, register r = query m = 4 q4 + r
                const int m = q4 * 4 + r;
                const int keyA = c - 15 + m, keyB = c + m + 1;
                if (keyA >= 0) *reinterpret_cast<__bf16*>(s3 + (keyA * FB_S3_LD + it * 16 + m) * 2) = (__bf16)XA[r];
                if (keyB <= 15) *reinterpret_cast<__bf16*>(s3 + (keyB * FB_S3_LD + it * 16 + m) * 2) = (__bf16)XB[r];
            }
        }
        // ---- S = (Q+u) K^T, dP = dO V^T : lane (key c, q4) holds queries il = 16 it + 4 q4 + r
        f4 S[4], dP[4];
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            S[it] = (f4){0.f, 0.f, 0.f, 0.f};
            dP[it] = (f4){0.f, 0.f, 0.f, 0.f};
            const int row = it * 16 + c;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                S[it] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa_frag(sQu, row, ks, q4), Kf[ks], S[it], 0, 0, 0);
                dP[it] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa_frag(sdO, row, ks, q4), Vf[ks], dP[it], 0, 0, 0);
            }
        }
        fb_lds_fence();
        bf8 Pdf[2], dSf[2];
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            union { uint2 u; __bf16 e[4]; } bd;
            bd.u = *reinterpret_cast<const uint2*>(s3 + (c * FB_S3_LD + it * 16 + q4 * 4) * 2);
            const float4 ls = *reinterpret_cast<const float4*>(sL + it * 16 + q4 * 4);
            const float4 dd = *reinterpret_cast<const float4*>(sL + 64 + it * 16 + q4 * 4);
            const float lsv[4] = {ls.x, ls.y, ls.z, ls.w}, ddv[4] = {dd.x, dd.y, dd.z, dd.w};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = I0 + it * 16 + q4 * 4 + r;
                const float s = (S[it][r] + (float)bd.e[r]) * a.scale;
                // the exponential unconditionally, then the select: behind a branch this kernel spills 4 to 12 B per lane more
                const float e = __expf(s - lsv[r]);
                const float p = admitted(i) ? e : 0.f;
                float g = dP[it][r], pd = p;
                if (a.thr > 0) {
                    const unsigned rnd = (fa_keep_rand4(a.seed, bh, T, i, j >> 2) >> (8 * (j & 3))) & 0xFFu;
                    const bool keep = rnd >= a.thr;
                    g = keep ? g * a.keep_scale : 0.f;
                    pd = keep ? p * a.keep_scale : 0.f;
                }
                const float ds = p * (g - ddv[r]) * a.scale;
                Pdf[it >> 1][(it & 1) * 4 + r] = (__bf16)pd;
                dSf[it >> 1][(it & 1) * 4 + r] = (__bf16)ds;
            }
        }
        // ---- dV^T += dO^T Pd ,  dK^T += (Q+u)^T dS : contraction over the tile's 64 queries
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const int qq = c >> 2, p = c & 3;
                const int rowA = kk * 32 + q4 * 4 + qq;
                const bf8 gf = fa_tr_pair(sdO, rowA, rowA + 16, mt * 2 + (p >> 1), p & 1);
                const bf8 qf = fa_tr_pair(sQu, rowA, rowA + 16, mt * 2 + (p >> 1), p & 1);
                dV[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gf, Pdf[kk], dV[mt], 0, 0, 0);
                dK[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf, dSf[kk], dK[mt], 0, 0, 0);
            }
        __syncthreads();
        if (t + 1 < qtiles.end) {
            commit();
            __syncthreads();
        }
    }
    if (j < T) {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            fa_store_head4(dkrow, mt, q4, dk, dK[mt]);
            fa_store_head4(dvrow, mt, q4, dk, dV[mt]);
        }
    }
}

// host: the backward under one span, after the entry point's argument checks: both kernels, the bias-partials pass and the
// position gradient.  dBand [H, B*T, rs] holds relative positions 0 .. 2c (c = the span's centre: sp.w under the full and local
// spans, T - 1 under the context span) behind p0 columns; they go to rows 0 .. 2c of dpl [pl_rows, d], zero rows behind them.
template <class Span>
int fb_backward(const void* qkv, const __bf16* pl, const float* bias_u, const float* bias_v, const int64_t* lens, const void* ctx,
                const void* dctx, const float* lse, int B, int T, int H, int dk, FaSpanArgs sp, int centre, int rs, int p0, float dropout_p, unsigned seed,
                void* dqkv, __bf16* dpl, int pl_rows, float* dbias_u, float* dbias_v, void* dBand, void* QvHM, float* ws,
                ia_stream_t stream) {
    const FbWs lay = fb_ws_layout(B, T, H, dk, rs);
    FbArgs a;
    a.qkv = (const __bf16*)qkv; a.pl = pl; a.bias_u = bias_u; a.bias_v = bias_v; a.lens = lens;
    a.ctx = (const __bf16*)ctx; a.dctx = (const __bf16*)dctx; a.lse = lse; a.dqkv = (__bf16*)dqkv; a.dBand = (__bf16*)dBand;
    a.QvHM = (__bf16*)QvHM; a.D = ws + lay.D; a.part = ws + lay.part; a.B = B; a.T = T; a.H = H; a.dk = dk; a.w = sp.w;
    a.w2 = sp.w2; a.chunk = sp.chunk;
    a.Rs = rs; a.pad0 = p0;
    a.scale = 1.f / sqrtf((float)dk); a.seed = seed;
    const ia_dropout_t drop = ia_dropout_rule(dropout_p);
    a.thr = drop.thr; a.keep_scale = drop.keep_scale;
    hipStream_t st = (hipStream_t)stream;
    // band columns no (wave, tile) flushes (keys beyond the length or the window, rows of padded queries) stay zero
    if (hipMemsetAsync(dBand, 0, (size_t)H * B * T * rs * sizeof(__bf16), st) != hipSuccess) return IA_LAUNCH_FAILED;
    const int nt = (T + 63) / 64;
    const int grid = 8 * ((B * H + 7) / 8) * nt;
    const bool full = (dk == 64);
    int rc = fa_launch<FbArgs, relpos_flash_bwd_q_kernel<true, Span>, relpos_flash_bwd_q_kernel<false, Span>>(full, grid, FB_Q_LDS, st, a);
    if (rc != IA_OK) return rc;
    rc = fa_launch<FbArgs, relpos_flash_bwd_kv_kernel<true, Span>, relpos_flash_bwd_kv_kernel<false, Span>>(full, grid, FB_KV_LDS, st, a);
    if (rc != IA_OK) return rc;
    ia_partials_finish(a.part, B * nt, 2 * H * dk, H * dk, dbias_u, dbias_v, st);
    IA_RETURN_IF_LAUNCH_FAILED();
    // position-projection gradient: the band columns p0 .. p0 + 2 centre of the heads' TN GEMMs
    return fb_dpos_gemm_pack(dBand, QvHM, ws, lay, rs, p0, 2 * centre + 1, B, T, H, dk, dpl, pl_rows, stream);
}

inline int fb_window(int T, int window) { return window < T - 1 ? window : T - 1; }   // a window beyond T - 1 admits no further key

}  // namespace

extern "C" int ia_relpos_attention_flash_bwd_dims(int T, int* Rs, int* pad0) {
    if (T <= 0 || !Rs || !pad0) return IA_INVALID_VALUE;
    const int p0 = (8 - ((T + 8 * 16 - 16) % 8)) % 8;          // (T - 16 + pad0) % 8 == 0: every wave's band starts on a 16-byte column
    const int nkt = (T + 63) / 64;
    *pad0 = p0;
    *Rs = (T - 16 + p0 + 64 * nkt + 16 + 7) / 8 * 8;           // largest flushed column + 1 (first wave, last key tile + carry)
    if (*Rs < p0 + 2 * T - 1) *Rs = (p0 + 2 * T - 1 + 7) / 8 * 8;
    return IA_OK;
}

extern "C" int64_t ia_relpos_attention_flash_bwd_ws_elems(int B, int T, int H, int dk) {
    int rs, p0;
    if (B <= 0 || T <= 0 || H <= 0 || dk <= 0) return 0;
    ia_relpos_attention_flash_bwd_dims(T, &rs, &p0);
    return fb_ws_layout(B, T, H, dk, rs).total;
}

extern "C" int ia_relpos_attention_flash_bwd(const void* qkv, const void* pos_proj, const float* bias_u, const float* bias_v,
                                             const int64_t* lens, const void* ctx, const void* dctx, const float* lse, int B,
                                             int T, int H, int dk, float dropout_p, unsigned seed, void* dqkv, void* dpl,
                                             int pl_rows, float* dbias_u, float* dbias_v, void* dBand, void* QvHM, float* ws,
                                             ia_stream_t stream) {
    if (!qkv || !pos_proj || !bias_u || !bias_v || !lens || !ctx || !dctx || !lse || !dqkv || !dpl || !dBand || !QvHM || !ws ||
        !dbias_u || !dbias_v || B <= 0 || T <= 0 || H <= 0 || pl_rows < 2 * T - 1)
        return IA_INVALID_VALUE;
    if (!ia_relpos_attention_flash_supported(T, dk)) return IA_UNSUPPORTED;
    if (dropout_p < 0.f || dropout_p >= 1.f) return IA_INVALID_VALUE;
    if (!ia_is_aligned(qkv, 16) || !ia_is_aligned(pos_proj, 16) || !ia_is_aligned(ctx, 8) || !ia_is_aligned(dctx, 8) ||
        !ia_is_aligned(dqkv, 8) || !ia_is_aligned(dBand, 16) || !ia_is_aligned(QvHM, 16) || !ia_is_aligned(ws, 16) ||
        !ia_is_aligned(dpl, 8))
        return IA_INVALID_VALUE;
    int rs, p0;
    ia_relpos_attention_flash_bwd_dims(T, &rs, &p0);
    return fb_backward<FaFullSpan>(qkv, (const __bf16*)pos_proj, bias_u, bias_v, lens, ctx, dctx, lse, B, T, H, dk, FaSpanArgs{T - 1, 0, 0}, T - 1, rs,
                                   p0, dropout_p, seed, dqkv, (__bf16*)dpl, pl_rows, dbias_u, dbias_v, dBand, QvHM, ws, stream);
}

extern "C" int ia_relpos_attention_local_bwd_dims(int T, int window, int* Rs, int* pad0) {
    if (T <= 0 || window <= 0 || !Rs || !pad0) return IA_INVALID_VALUE;
    const int w = fb_window(T, window);
    const int p0 = (8 - (w + 1) % 8) % 8;         // (w - 15 - iw + pad0) % 8 == 0: every flushed chunk starts on a 16-byte column
    *pad0 = p0;
    *Rs = (p0 + 2 * w + 1 + 7) / 8 * 8;           // relative positions 0 .. 2w behind pad0: no term in T
    return IA_OK;
}

extern "C" int64_t ia_relpos_attention_local_bwd_ws_elems(int B, int T, int H, int dk, int window) {
    int rs, p0;
    if (B <= 0 || H <= 0 || dk <= 0 || ia_relpos_attention_local_bwd_dims(T, window, &rs, &p0) != IA_OK) return 0;
    return fb_ws_layout(B, T, H, dk, rs).total;
}

extern "C" int ia_relpos_attention_local_bwd(const void* qkv, const void* pos_proj, const float* bias_u, const float* bias_v,
                                             const int64_t* lens, const void* ctx, const void* dctx, const float* lse, int B,
                                             int T, int H, int dk, int window, float dropout_p, unsigned seed, void* dqkv,
                                             void* dpl, int pl_rows, float* dbias_u, float* dbias_v, void* dBand, void* QvHM,
                                             float* ws, ia_stream_t stream) {
    if (!qkv || !pos_proj || !bias_u || !bias_v || !lens || !ctx || !dctx || !lse || !dqkv || !dpl || !dBand || !QvHM || !ws ||
        !dbias_u || !dbias_v || B <= 0 || T <= 0 || H <= 0 || window <= 0 || (int64_t)pl_rows < 2 * (int64_t)window + 1)
        return IA_INVALID_VALUE;
    if (!ia_relpos_attention_local_supported(T, dk, window)) return IA_UNSUPPORTED;
    if (dropout_p < 0.f || dropout_p >= 1.f) return IA_INVALID_VALUE;
    if (!ia_is_aligned(qkv, 16) || !ia_is_aligned(pos_proj, 16) || !ia_is_aligned(ctx, 8) || !ia_is_aligned(dctx, 8) ||
        !ia_is_aligned(dqkv, 8) || !ia_is_aligned(dBand, 16) || !ia_is_aligned(QvHM, 16) || !ia_is_aligned(ws, 16) ||
        !ia_is_aligned(dpl, 8))
        return IA_INVALID_VALUE;
    // as the forward: the band of w' = min(window, T - 1) on the table advanced by window - w' rows; so are dpl's rows, and the
    // rows in front of them are zero
    const int w = fb_window(T, window), row0 = window - w;
    const size_t d = (size_t)H * dk;
    int rs, p0;
    ia_relpos_attention_local_bwd_dims(T, window, &rs, &p0);
    if (row0 > 0 && hipMemsetAsync(dpl, 0, (size_t)row0 * d * sizeof(__bf16), (hipStream_t)stream) != hipSuccess) return IA_LAUNCH_FAILED;
    return fb_backward<FaLocalSpan>(qkv, (const __bf16*)pos_proj + (size_t)row0 * d, bias_u, bias_v, lens, ctx, dctx, lse, B, T, H, dk,
                                    FaSpanArgs{w, 0, 0}, w, rs, p0, dropout_p, seed, dqkv, (__bf16*)dpl + (size_t)row0 * d, pl_rows - row0, dbias_u, dbias_v, dBand,
                                    QvHM, ws, stream);
}

// ---- limited context: the full span's dBand layout and workspace (kBoundedBand = false), the context span's pairs
extern "C" int ia_relpos_attention_context_bwd_dims(int T, int style, int left, int right, int* Rs, int* pad0) {
    FaSpanArgs sp;
    if (!Rs || !pad0 || fa_context_args(T, style, left, right, &sp) == FA_CTX_INVALID) return IA_INVALID_VALUE;
    return ia_relpos_attention_flash_bwd_dims(T, Rs, pad0);
}

extern "C" int64_t ia_relpos_attention_context_bwd_ws_elems(int B, int T, int H, int dk, int style, int left, int right) {
    FaSpanArgs sp;
    if (fa_context_args(T, style, left, right, &sp) == FA_CTX_INVALID) return 0;
    return ia_relpos_attention_flash_bwd_ws_elems(B, T, H, dk);
}

extern "C" int ia_relpos_attention_context_bwd(const void* qkv, const void* pos_proj, const float* bias_u, const float* bias_v,
                                               const int64_t* lens, const void* ctx, const void* dctx, const float* lse, int B,
                                               int T, int H, int dk, int style, int left, int right, float dropout_p,
                                               unsigned seed, void* dqkv, void* dpl, int pl_rows, float* dbias_u, float* dbias_v,
                                               void* dBand, void* QvHM, float* ws, ia_stream_t stream) {
    if (!qkv || !pos_proj || !bias_u || !bias_v || !lens || !ctx || !dctx || !lse || !dqkv || !dpl || !dBand || !QvHM || !ws ||
        !dbias_u || !dbias_v || B <= 0 || T <= 0 || H <= 0 || pl_rows < 2 * T - 1)
        return IA_INVALID_VALUE;
    FaSpanArgs sp;
    const int kind = fa_context_args(T, style, left, right, &sp);
    if (kind == FA_CTX_INVALID) return IA_INVALID_VALUE;
    if (!ia_relpos_attention_flash_supported(T, dk)) return IA_UNSUPPORTED;
    if (dropout_p < 0.f || dropout_p >= 1.f) return IA_INVALID_VALUE;
    if (!ia_is_aligned(qkv, 16) || !ia_is_aligned(pos_proj, 16) || !ia_is_aligned(ctx, 8) || !ia_is_aligned(dctx, 8) ||
        !ia_is_aligned(dqkv, 8) || !ia_is_aligned(dBand, 16) || !ia_is_aligned(QvHM, 16) || !ia_is_aligned(ws, 16) ||
        !ia_is_aligned(dpl, 8))
        return IA_INVALID_VALUE;
    int rs, p0;
    ia_relpos_attention_flash_bwd_dims(T, &rs, &p0);
    if (kind == FA_CTX_FULL)   // every pair admitted: the full span's kernels and bits
        return fb_backward<FaFullSpan>(qkv, (const __bf16*)pos_proj, bias_u, bias_v, lens, ctx, dctx, lse, B, T, H, dk, FaSpanArgs{T - 1, 0, 0},
                                       T - 1, rs, p0, dropout_p, seed, dqkv, (__bf16*)dpl, pl_rows, dbias_u, dbias_v, dBand, QvHM, ws, stream);
    return fb_backward<FaContextSpan>(qkv, (const __bf16*)pos_proj, bias_u, bias_v, lens, ctx, dctx, lse, B, T, H, dk, sp, T - 1, rs, p0,
                                      dropout_p, seed, dqkv, (__bf16*)dpl, pl_rows, dbias_u, dbias_v, dBand, QvHM, ws, stream);
}
