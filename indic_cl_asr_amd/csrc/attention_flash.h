// The key-tiled rel-pos attention kernels' one vocabulary.  There is one kernel template per role, written once as
// template <bool DK64, class Span>: the forward (attention_flash.hip), the query-owner and the key-owner backward
// (attention_flash_bwd.hip).  Full attention, local attention (|i - j| <= w) and a limited context under full rel-pos attention
// (regular [L, R] or chunked_limited) are the same kernels under three spans; the Span section below lists everything in which
// they differ.  Here: fragment types, tile constants, the attention-dropout hash (the
// backward regenerates the forward's mask), the zero-padding head-row loader, the swizzled LDS addresses and fragment reads,
// register staging of a tile (fetch / commit), the spans, the K | V | P stage, the query fragments, the band block, the workgroup
// coordinates, the guarded head-row store, the backwards' strip geometry, workspace layout and position-gradient step, and the
// host's launch of a <DK64> pair.  tests/test_attention_flash_digests_gpu.py pins the bits of everything the kernels build from
// it under the full span, tests/test_attention_local_digests_gpu.py under the local one.
#pragma once
#include <hip/hip_bf16.h>

#include "dropout_mask.h"
#include "ia_common.h"

namespace {

typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
typedef short s4v __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int FA_THREADS = 256;
constexpr int FA_ROWB = 128;               // bytes per LDS row (64 bf16, zero-padded beyond dk)
constexpr int FA_T64 = 64 * FA_ROWB;       // a 64-row tile: 8 KB
constexpr int FA_PBUF = 128 * FA_ROWB;     // 128 position rows: 16 KB
constexpr int FA_SR_LD = 104;              // bf16 elements per forward band-strip row (208 B: conflict-free 8-byte reads)

// attention-dropout randomness of these kernels: one word per (head, query, group of 4 keys); key j uses byte j & 3.  The
// word comes from dropout_mask.h's full-rate construction (24-bit multiplies, shifts, xors): the 32-bit multiplies of a
// murmur-style finaliser are quarter rate on gfx950 and the forward regenerates 16 words per wave and key tile.
__device__ __forceinline__ unsigned fa_keep_rand4(unsigned seed, int bh, int T, int i, int j4) {
    const unsigned idx = ((unsigned)bh * (unsigned)T + (unsigned)i) * (unsigned)((T + 3) >> 2) + (unsigned)j4;
    return ia_dm_word24(ia_dm_hash32(seed), idx);   // (the seed hash is wave-uniform: hoisted to scalar code)
}

// 16-byte slot `slot` (8 elements) of a head row of `dk` elements starting at `row` (8-byte aligned), zero beyond dk
template <bool FULL>
__device__ __forceinline__ uint4 fa_load_slot(const __bf16* row, int slot, int dk) {
    if constexpr (FULL) {
        return *reinterpret_cast<const uint4*>(row + slot * 8);
    } else {
        uint4 v = make_uint4(0, 0, 0, 0);
        const int e0 = slot * 8;
        if (e0 < dk) { const uint2 a = *reinterpret_cast<const uint2*>(row + e0); v.x = a.x; v.y = a.y; }
        if (e0 + 4 < dk) { const uint2 a = *reinterpret_cast<const uint2*>(row + e0 + 4); v.z = a.x; v.w = a.y; }
        return v;
    }
}

// 16-byte slot `slot` of row `row` of an LDS tile: these kernels' own swizzle, slot ^ (row & 7)
template <typename B>
__device__ __forceinline__ B* fa_swz(B* tile, int row, int slot) { return tile + row * FA_ROWB + ((slot ^ (row & 7)) * 16); }

// row-major MFMA fragment: elements 32 ks + 8 q4 .. + 7 of row `row`
__device__ __forceinline__ bf8 fa_frag(const unsigned char* tile, int row, int ks, int q4) {
    return *reinterpret_cast<const bf8*>(fa_swz(tile, row, ks * 4 + q4));
}

// transposed MFMA fragment by two ds_read_b64_tr_b16: 8-byte half `half` of slot `sl` of rows rowA (elements 0 .. 3) and rowB
__device__ __forceinline__ bf8 fa_tr_pair(const unsigned char* tile, int rowA, int rowB, int sl, int half) {
    typedef __attribute__((address_space(3))) s4v lds_s4v;
    const s4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4v*)(fa_swz(tile, rowA, sl) + half * 8));
    const s4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4v*)(fa_swz(tile, rowB, sl) + half * 8));
    union { s4v s[2]; bf8 v; } f;
    f.s[0] = lo; f.s[1] = hi;
    return f.v;
}

// ---- register staging: thread tid holds slot idx & 7 of tile row idx >> 3, idx = tid + i * 256, i < N (N = rows / 32).  The
// tile's row `row` is the global row base + clamp(row0 + row) * stride, clamped to <= hi and, with LOW, to >= 0.
template <bool DK64, bool LOW, int N>
__device__ __forceinline__ void fa_fetch_rows(uint4 (&r)[N], const __bf16* base, int stride, int row0, int hi, int dk, int tid) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int idx = tid + i * FA_THREADS, row = idx >> 3, sl = idx & 7;
        int g = row0 + row;
        if constexpr (LOW) g = g < 0 ? 0 : (g > hi ? hi : g);
        else g = g > hi ? hi : g;
        r[i] = fa_load_slot<DK64>(base + (size_t)g * stride, sl, dk);
    }
}

template <int N>
__device__ __forceinline__ void fa_commit_rows(unsigned char* tile, const uint4 (&r)[N], int tid) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int idx = tid + i * FA_THREADS, row = idx >> 3, sl = idx & 7;
        *reinterpret_cast<uint4*>(fa_swz(tile, row, sl)) = r[i];
    }
}

// ---- Span: which (query, key) pairs exist.  A small device-side value; FaFullSpan admits every key below the length,
// FaLocalSpan the keys |i - j| <= w below the length (0 <= w <= T - 1: the host reduces a larger window), FaContextSpan one
// interval of keys per query on the full span's position table (below).  Every span is built from (T, FaSpanArgs) and reads of
// the three integers what it needs.  It supplies what differs between the attention models, and nothing else.  The owner of a
// walk is named by a tag, FaQueryOwner (forward, query-owner backward: a query tile walks key tiles, a query admits keys) or
// FaKeyOwner (key-owner backward: a key tile walks query tiles, a key admits queries); the two symmetric spans ignore it.
//   1. centre(): the position row of relative position 0, T - 1 (full, context) or w (local).  The stage's position rows are
//      centre - I0 - 63 + j0 .. + 127 clamped to [0, 2 centre] (clamped rows give finite band values for pairs that the
//      admissibility removes), the key-owner's centre - i0 - 63 + J0 .. + 127, and the dBand column of strip column 0 is
//      centre - 15 - iw + j0 + pad0.
//   2. tiles(owner, X0, len): the 64-row tiles lo .. end - 1 of the OTHER axis that a query tile or key tile at X0 < len walks.  Full:
//      every tile below len.  Local: those that hold a row of [max(X0 - w, 0), min(X0 + 63 + w, len - 1)] (both ends
//      non-negative, the first <= X0 <= the second), 1 + 2 ceil(w / 64) tiles at the most whatever T is.  The one-stage prefetch
//      follows them.  A plain aggregate read by its members, walked `t < end`, `t + 1 < end`: that is the form in which the full
//      forward compiles to its earlier loop (walked `t <= last`, or through member functions, it is 1 % slower at T = 3001;
//      profiles/attention_span_refactor.md).
//   3. admit(owner, own, valid, len): the rows of the other axis that pair with a lane's own row, built once per lane and asked once per
//      element.  `valid` is own < len; the forward passes true (a padded query's context is zeroed at the store).  In the backward
//      an inadmissible pair gives P = 0 by value, in the forward -inf before the row maximum.
//   4. tile_unmasked(j0, iw, len): the forward's mask-free score branch.  Full: the key tile lies below len (workgroup-uniform).
//      Local: it also lies inside the window of all 16 queries iw .. iw + 15 of the wave (per wave).
//   5. Two compile-time facts, the points where the spans differ in output bits or in stores:
//      kSparseTiles: a processed tile may hold no admissible key for a query (the tile left of the diagonal at a small w, a
//        padded query).  Running and new maximum are then both -inf, so the forward takes its exponentials against 0 (exp2(-inf)
//        = 0, no NaN) and zeroes a padded query's accumulator BY VALUE.  The full span uses the new maximum directly (finite: key
//        j0 < len exists in every processed tile) and stores O * 0, which is -0.0 for a negative accumulator.
//      kBoundedBand: the dBand row holds only [0, Rs), Rs = ceil8(pad0 + 2w + 1) whatever T is, and strip columns outside it
//        (exact zeros of inadmissible pairs) are dropped chunk by chunk, the final carry included.  The full span's row holds
//        every flushed column; only a partial last wave's leading chunks fall left of column 0.
// Aggregates are returned by value: filled through a reference under control flow they cost the query-owner registers.
struct FaTiles { int lo, end; };   // tiles lo .. end - 1
struct FaSpanArgs { int w, w2, chunk; };   // local: w.  context: regular (L, R, 0) or chunked (n, -, C).  full: unread
struct FaQueryOwner {};
struct FaKeyOwner {};

struct FaFullSpan {
    static constexpr bool kSparseTiles = false, kBoundedBand = false;
    struct Adm {
        bool ok; int len;
        __device__ __forceinline__ bool operator()(int x) const { return ok && x < len; }
    };
    int T;
    __device__ __forceinline__ FaFullSpan(int T_, const FaSpanArgs&) : T(T_) {}
    __device__ __forceinline__ int centre() const { return T - 1; }
    template <class Owner>
    __device__ __forceinline__ FaTiles tiles(Owner, int, int len) const { return FaTiles{0, (len + 63) / 64}; }
    template <class Owner>
    __device__ __forceinline__ Adm admit(Owner, int, bool valid, int len) const { return Adm{valid, len}; }
    __device__ __forceinline__ bool tile_unmasked(int j0, int, int len) const { return j0 + 64 <= len; }
};

struct FaLocalSpan {
    static constexpr bool kSparseTiles = true, kBoundedBand = true;
    struct Adm {   // [lo, hi], empty (lo = len > hi) for an own row >= len
        int lo, hi;
        __device__ __forceinline__ bool operator()(int x) const { return x >= lo && x <= hi; }
    };
    int w;
    __device__ __forceinline__ FaLocalSpan(int, const FaSpanArgs& s) : w(s.w) {}
    __device__ __forceinline__ int centre() const { return w; }
    template <class Owner>
    __device__ __forceinline__ FaTiles tiles(Owner, int X0, int len) const {
        const int lo = X0 - w > 0 ? X0 - w : 0, hi = X0 + 63 + w < len - 1 ? X0 + 63 + w : len - 1;
        return FaTiles{lo / 64, hi / 64 + 1};
    }
    template <class Owner>
    __device__ __forceinline__ Adm admit(Owner, int own, bool valid, int len) const {
        return Adm{valid ? own - w : len, own + w < len - 1 ? own + w : len - 1};
    }
    __device__ __forceinline__ bool tile_unmasked(int j0, int iw, int len) const {
        return j0 + 64 <= len && j0 >= iw + 15 - w && j0 + 63 <= iw + w;
    }
};

// A limited context under full rel-pos attention: the reference encoder's att_context_size = [L, R] with att_context_style
// 'regular' or 'chunked_limited' (A/modules/conformer_encoder.py:686-740, a [T, T] mask there).  The keys of a query are ONE
// interval and so are the queries of a key; the position table is the full span's (2T - 1 rows, centre T - 1):
//   regular [L, R]            keys of i: [i - L, i + R]                        queries of j: [j - R, j + L]
//   chunked, C = R + 1,       keys of i: [(i/C - n) C, (i/C + 1) C - 1]        queries of j: [(j/C) C, (j/C + n + 1) C - 1]
//     n = L / C
// The host reduces every form to these two with bounded integers: an unlimited side of a regular context is T, chunked
// [L, -1] is regular [L, T], C is at most T and n at most (T - 1) / C (so n C <= T - 1: no overflow for T < 2^29).  chunk == 0
// selects the regular form, (w, w2) = (L, R); chunk = C > 0 the chunked one, w = n.
//   tiles(owner, X0, len): the tiles that hold a row of [lo(X0), hi(min(X0 + 63, len - 1))] clamped to [0, len - 1], lo / hi the
//     owner's interval ends (both monotone in the row; lo(x) <= x <= hi(x), so the range is never empty).  Only these are
//     visited: O(T (L + R)) work when both sides are limited.
//   tile_unmasked: the key tile lies below len, at or right of the first key of query iw + 15 and at or left of the last key of
//     query iw: inside the interval of all 16 queries of the wave, by monotonicity, under either style.
//   kSparseTiles: a visited tile can hold no key for a query (everything right of the diagonal under [L, 0], a chunk edge
//     inside a tile), so the all-masked guard and the by-value zero apply as under the local span.
//   kBoundedBand = false: the backward keeps the FULL span's dBand layout (ia_relpos_attention_flash_bwd_dims' Rs and pad0,
//     every flushed column written, the memset's zeros elsewhere) and the position gradient contracts all 2T - 1 rows.  A
//     bounded band for this span is not built.
struct FaContextSpan {
    static constexpr bool kSparseTiles = true, kBoundedBand = false;
    struct Adm {   // [lo, hi], empty (lo = len > hi) for an own row >= len
        int lo, hi;
        __device__ __forceinline__ bool operator()(int x) const { return x >= lo && x <= hi; }
    };
    int T, a, b, C;
    __device__ __forceinline__ FaContextSpan(int T_, const FaSpanArgs& s) : T(T_), a(s.w), b(s.w2), C(s.chunk) {}
    __device__ __forceinline__ int centre() const { return T - 1; }
    // first and last row of the other axis that pair with row x of the owner's (not clamped to the utterance)
    __device__ __forceinline__ int lo(FaQueryOwner, int x) const { return C > 0 ? (x / C - a) * C : x - a; }
    __device__ __forceinline__ int hi(FaQueryOwner, int x) const { return C > 0 ? (x / C + 1) * C - 1 : x + b; }
    __device__ __forceinline__ int lo(FaKeyOwner, int x) const { return C > 0 ? (x / C) * C : x - b; }
    __device__ __forceinline__ int hi(FaKeyOwner, int x) const { return C > 0 ? (x / C + a + 1) * C - 1 : x + a; }
    template <class Owner>
    __device__ __forceinline__ FaTiles tiles(Owner o, int X0, int len) const {
        const int l = lo(o, X0), h = hi(o, X0 + 63 < len - 1 ? X0 + 63 : len - 1);
        return FaTiles{(l > 0 ? l : 0) / 64, (h < len - 1 ? h : len - 1) / 64 + 1};
    }
    template <class Owner>
    __device__ __forceinline__ Adm admit(Owner o, int own, bool valid, int len) const {
        const int l = lo(o, own), h = hi(o, own);
        return Adm{valid ? l : len, h < len - 1 ? h : len - 1};
    }
    __device__ __forceinline__ bool tile_unmasked(int j0, int iw, int len) const {
        return j0 + 64 <= len && j0 >= lo(FaQueryOwner{}, iw + 15) && j0 + 63 <= hi(FaQueryOwner{}, iw);
    }
};

// The K | V | P stage of the forward and the query-owner (32 KB at `smem`): key tile t of one (utterance, head), rows clamped to
// T - 1, and the 128 position rows centre - I0 - 63 + 64 t .. + 127 that cover the bands of the four waves of query tile I0,
// clamped to [0, 2 centre].  fetch(t) brings tile t to registers (8 x 16 B per thread), commit() writes them to LDS.
template <bool DK64>
struct FaKvpStage {
    uint4 rk[2], rv[2], rp[4];
    const __bf16 *kbase, *vbase, *pbase;
    unsigned char* smem;
    int T, d, dk, I0, centre, tid;
    __device__ __forceinline__ FaKvpStage(const __bf16* qkv, const __bf16* pl, unsigned char* smem_, int b, int h, int T_, int d_,
                                          int dk_, int I0_, int centre_, int tid_)
        : kbase(qkv + (size_t)b * T_ * (3 * d_) + d_ + h * dk_), vbase(kbase + d_), pbase(pl + h * dk_), smem(smem_), T(T_), d(d_),
          dk(dk_), I0(I0_), centre(centre_), tid(tid_) {}
    __device__ __forceinline__ void fetch(int t) {
        const int j0 = t * 64;
        fa_fetch_rows<DK64, false>(rk, kbase, 3 * d, j0, T - 1, dk, tid);
        fa_fetch_rows<DK64, false>(rv, vbase, 3 * d, j0, T - 1, dk, tid);
        fa_fetch_rows<DK64, true>(rp, pbase, d, centre - I0 - 63 + j0, 2 * centre, dk, tid);
    }
    __device__ __forceinline__ void commit() {
        fa_commit_rows(smem, rk, tid);
        fa_commit_rows(smem + FA_T64, rv, tid);
        fa_commit_rows(smem + 2 * FA_T64, rp, tid);
    }
};

// k-step ks of the B fragments (q+u)^T and (q+v)^T of the lane's query row `qrow` (head h's slice): lane (query c, q4) holds dk
// elements 32 ks + 8 q4 .. + 7
template <bool DK64>
__device__ __forceinline__ void fa_query_frags(const __bf16* qrow, const float* bias_u, const float* bias_v, int h, int dk, int ks,
                                               int q4, bf8& Qu, bf8& Qv) {
    union { uint4 u; __bf16 e[8]; } q;
    q.u = fa_load_slot<DK64>(qrow, ks * 4 + q4, dk);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int e = ks * 32 + q4 * 8 + j;
        const float u = (e < dk) ? bias_u[h * dk + e] : 0.f, v = (e < dk) ? bias_v[h * dk + e] : 0.f;
        Qu[j] = (__bf16)((float)q.e[j] + u);
        Qv[j] = (__bf16)((float)q.e[j] + v);
    }
}

// band R^T = P_band (q+v)^T [80 positions x 16 queries] of one wave, 5 x 2 MFMAs: rows = staged position rows pw0 + 16 rt + c,
// columns = queries; then the skew through the wave's strip: strip[query c][rr + c + 1] = R^T[rr][c]  (rr = 16 rt + 4 q4 + r), so
// that the band element of key tile column jl is at strip column jl + 16
__device__ __forceinline__ void fa_band_to_strip(const unsigned char* sP, unsigned char* sR, int pw0, const bf8 (&Qv)[2], int c,
                                                 int q4) {
    f4 R[5];
#pragma unroll
    for (int rt = 0; rt < 5; ++rt) {
        R[rt] = (f4){0.f, 0.f, 0.f, 0.f};
        const int row = pw0 + rt * 16 + c;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
            R[rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa_frag(sP, row, ks, q4), Qv[ks], R[rt], 0, 0, 0);
    }
#pragma unroll
    for (int rt = 0; rt < 5; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            *reinterpret_cast<__bf16*>(sR + (c * FA_SR_LD + rt * 16 + q4 * 4 + r + c + 1) * 2) = (__bf16)R[rt][r];
}

// Workgroup coordinates of all three kernels: (utterance b, head h, 64-row tile) and the utterance's length clamped to [0, T].
// XCD-aware order: the tiles of one (utterance, head) share K / V / position rows, so their workgroup ids are congruent mod 8.
// Returned by value: filled through a reference with an early return it costs the query-owner 4 VGPRs and 120 instructions.
struct FaWg { int bh, tile, h, b, len; };   // len < 0: no such (utterance, head)
__device__ __forceinline__ FaWg fa_wg(int B, int T, int H, const int64_t* lens) {
    const int nt = (T + 63) / 64;
    const int xcd = blockIdx.x & 7, slot_id = blockIdx.x >> 3;
    const int bh = xcd + 8 * (slot_id / nt);
    FaWg w{bh, slot_id % nt, bh % H, bh / H, -1};
    if (bh < B * H) {
        const int len = (int)lens[w.b];
        w.len = len < 0 ? 0 : (len > T ? T : len);
    }
    return w;
}

// elements 16 mt + 4 q4 .. + 3 of a head row as bf16, if they exist (dk is a multiple of 4)
__device__ __forceinline__ void fa_store_head4(__bf16* row, int mt, int q4, int dk, f4 x, float scale = 1.f) {
    if (mt * 16 + q4 * 4 < dk) {
        union { uint2 u; __bf16 e[4]; } o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o.e[r] = (__bf16)(x[r] * scale);
        *reinterpret_cast<uint2*>(row + mt * 16 + q4 * 4) = o.u;
    }
}

// ---- the backward's (attention_flash_bwd.hip): strip geometry, the strip fence, the workspace layout and the position-gradient
// step
constexpr int FB_SB_LD = 120;                 // dS band strip: columns [0,96) band rows of this tile, [96,112) carry
constexpr int FB_Q_STRIP = 16 * (FA_SR_LD + FB_SB_LD) * 2;           // per wave: 7168 B
constexpr int FB_Q_LDS = 2 * FA_T64 + FA_PBUF + 4 * FB_Q_STRIP;      // K | V | P | strips = 61 440 B
constexpr int FB_S3_LD = 72;                  // key-major band strip: [16 keys][64 queries (+8 pad)]
constexpr int FB_KV_STAGE = 3 * FA_T64 + FA_PBUF + 512;              // Qu | Qv | dO | P | lse[64] D[64]
constexpr int FB_KV_LDS = FB_KV_STAGE + 4 * 16 * FB_S3_LD * 2;       // 50 688 B

__device__ __forceinline__ void fb_lds_fence() {   // order this wave's LDS accesses across differently typed views of a strip
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// dpl[r][h*dk + e] = bf16(dpos[h][pad0 + r][e]) for r < R, zero rows beyond (dpos rows are [Rs*64 | Rs] f32 blocks: the TN GEMM's
// weight and bias gradient outputs, the latter unused)
__global__ __launch_bounds__(256) void fb_dpos_pack_kernel(const float* __restrict__ dpos, int H, int Rs, int pad0, int R, int dk,
                                                           int rows, __bf16* __restrict__ out) {
    const int d = H * dk, q = dk / 4;
    const int64_t total = (int64_t)rows * H * q;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int e4 = (int)(i % q);
        const int h = (int)((i / q) % H);
        const int r = (int)(i / ((int64_t)q * H));
        union { uint2 u; __bf16 e[4]; } o;
        o.u = make_uint2(0, 0);
        if (r < R) {
            const float4 v = *reinterpret_cast<const float4*>(dpos + (size_t)h * ((size_t)Rs * 64 + Rs) + (size_t)(pad0 + r) * 64 + e4 * 4);
            o.e[0] = (__bf16)v.x; o.e[1] = (__bf16)v.y; o.e[2] = (__bf16)v.z; o.e[3] = (__bf16)v.w;
        }
        *reinterpret_cast<uint2*>(out + (size_t)r * d + h * dk + e4 * 4) = o.u;
    }
}

// host: the backward's f32 workspace  part | D | dpos | tn  (element offsets) for a dBand row stride rs
struct FbWs { int64_t part, D, dpos, tn, total; };
inline FbWs fb_ws_layout(int B, int T, int H, int dk, int rs) {
    FbWs w;
    auto up = [](int64_t x) { return (x + 63) / 64 * 64; };
    w.part = 0;
    w.D = up((int64_t)B * ((T + 63) / 64) * 2 * H * dk);
    w.dpos = w.D + up((int64_t)B * H * T);
    w.tn = w.dpos + up((int64_t)H * ((int64_t)rs * 64 + rs));
    {
        ia_tn_problem pr[8];
        const int nh = H < 8 ? H : 8;
        for (int i = 0; i < nh; ++i) pr[i] = ia_tn_problem{nullptr, nullptr, nullptr, nullptr, rs, 64, B * T, rs, 64};
        w.total = w.tn + up(ia_gemm_tn_grouped_scratch_elems(pr, nh));
    }
    return w;
}

// host: position-projection gradient: per head dpos_h [rs, 64] = dBand_h^T (q+v)_h over the B*T rows (split-K TN GEMM), then the
// band columns pad0 .. pad0 + R - 1 go to rows 0 .. R - 1 of out [rows, d] bf16, zero rows behind them
inline int fb_dpos_gemm_pack(const void* dBand, const void* QvHM, float* ws, const FbWs& w, int rs, int p0, int R, int B, int T, int H,
                             int dk, void* out, int rows, ia_stream_t stream) {
    float* dpos = ws + w.dpos;
    for (int h0 = 0; h0 < H; h0 += 8) {   // the heads' TN GEMMs as grouped launches (one GEMM + one finishing pass per <= 8 heads)
        ia_tn_problem pr[8];
        const int nh = H - h0 < 8 ? H - h0 : 8;
        for (int i = 0; i < nh; ++i) {
            const int h = h0 + i;
            float* o = dpos + (size_t)h * ((size_t)rs * 64 + rs);
            pr[i] = ia_tn_problem{(const __bf16*)dBand + (size_t)h * B * T * rs, (const __bf16*)QvHM + (size_t)h * B * T * 64, o, nullptr,
                                  rs, 64, B * T, rs, 64};
        }
        const int rc = ia_gemm_tn_bf16_grouped(pr, nh, ws + w.tn, stream);
        if (rc != IA_OK) return rc;
    }
    const int64_t items = (int64_t)rows * H * (dk / 4);
    const int64_t blocks = (items + 255) / 256;
    hipLaunchKernelGGL(fb_dpos_pack_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream,
                       (const float*)dpos, H, rs, p0, R, dk, rows, (__bf16*)out);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}

// host: (style, left, right) of the limited-context entry points (style 0 regular, 1 chunked_limited; a side of -1 is unlimited)
// -> the context span's bounded integers.  FA_CTX_FULL: the context admits every pair (the caller runs the full span);
// FA_CTX_INVALID: unknown style, a side below -1, or chunked with left >= 0, right >= 0 and left % (right + 1) != 0.
enum { FA_CTX_INVALID = -1, FA_CTX_SPAN = 0, FA_CTX_FULL = 1 };
inline int fa_context_args(int T, int style, int left, int right, FaSpanArgs* sp) {
    if (T <= 0 || (style != 0 && style != 1) || left < -1 || right < -1) return FA_CTX_INVALID;
    if (style == 1 && right >= 0) {
        if (left >= 0 && left % (right + 1) != 0) return FA_CTX_INVALID;
        if (right + 1 >= T) return FA_CTX_FULL;   // one chunk holds every frame
        const int C = right + 1, nmax = (T - 1) / C;
        *sp = FaSpanArgs{(left < 0 || left / C > nmax) ? nmax : left / C, 0, C};
        return FA_CTX_SPAN;
    }
    // regular, and chunked [L, -1] (i - j <= L alone); i - j and j - i never exceed T - 1
    const int L = (left < 0 || left > T - 1) ? T - 1 : left, R = (right < 0 || right > T - 1) ? T - 1 : right;
    if (L == T - 1 && R == T - 1) return FA_CTX_FULL;
    *sp = FaSpanArgs{L, R, 0};
    return FA_CTX_SPAN;
}

// host: raise the kernel's LDS limit once, launch it on FA_THREADS threads, IA_LAUNCH_FAILED if either fails
template <typename Args, void (*KERNEL)(Args)>
inline int fa_launch_one(int grid, int lds, hipStream_t st, const Args& a) {
    IA_SET_MAX_LDS_ONCE(KERNEL, lds);
    hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(FA_THREADS), lds, st, a);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}
// host: the <true> (dk = 64, whole 16-byte slots) or the <false> (zero-padding) instantiation of a kernel template
template <typename Args, void (*FULL)(Args), void (*PADDED)(Args)>
inline int fa_launch(bool full, int grid, int lds, hipStream_t st, const Args& a) {
    return full ? fa_launch_one<Args, FULL>(grid, lds, st, a) : fa_launch_one<Args, PADDED>(grid, lds, st, a);
}

}  // namespace
