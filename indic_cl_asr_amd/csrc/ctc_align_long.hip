// CTC forced alignment of long transcripts for gfx950: ctc_viterbi (csrc/ctc_align.hip) spread over one WORKGROUP per utterance.
// Same definition, arithmetic order and tie-breaks (fp32; q = logit - lse first, then added; the first maximum of
// [stay, s-1, s-2] wins; L-2 beats L-1 at the end; L = 1 ends in state 0), so results are bit-equal to the one-wave kernel's and
// to align.ctc_forced_align_host.
//
//   ctc_viterbi_wg : W waves (1..16, a power of two), lane i of the workgroup owns the K consecutive states [i K, (i+1) K),
//                 K in {4, 8, 16}:  K = 4 up to L = 2S+1 <= 4096, then the smallest K with L <= 1024 K;  W the smallest power
//                 of two with L <= 64 K W.  (K, W) therefore changes after S = 127, 255, 511, 1023, 2047 and 4095; S <= 8191.
//                 K is even, so a lane's first state is a blank: it has no s-2 candidate, and the only value that crosses a
//                 lane is the predecessor's last state.  Inside a wave that is one DPP shift; across waves lane 63 publishes
//                 it to xw[t & 1][wave] after frame t and lane 0 of the next wave reads xw[(t-1) & 1][wave-1] at frame t:
//                 one workgroup barrier per frame, and nothing waits between workgroups.
//                 Even states all add q_t(blank): one broadcast load per frame; the K/2 token gathers of a lane are
//                 prefetched PF frames ahead.  prev[] is updated in place from j = K-1 downwards.
//   workspace   : 2 bits per state, the K of a lane packed into one word of 2K bits (u8 / u16 / u32); frame t of utterance b
//                 is the row of 64 W words at word index (b T + t) 64 W, lane i's word at column i: T * 64 W K / 4 bytes per
//                 utterance (= T * ceil(L/4) rounded up to the workgroup), written coalesced.
//   backtrace   : same launch, after a barrier, by wave 0.  The state falls by at most 2 per frame, so the next BT = 16 frames
//                 touch only the words [s/K - ceil(30/K), s/K]: lane (i, w) loads word s/K - w - 4r of frame t - i (r < NL
//                 registers), and the dependent chain per frame is readlane -> bit extract -> subtract on the scalar unit.
//                 The state of frame t is parked in lane t % 64; the path leaves in 64-frame rows.
//   spans       : after a second barrier, the whole workgroup over the path just written, one frame per thread.
#include "ia_common.h"

namespace {

constexpr int LONG_MAX_K = 16;
constexpr int LONG_MAX_S = (1024 * LONG_MAX_K - 1) / 2;   // L = 2S+1 <= 1024 K

struct LongWs { int K, waves; size_t total; };

static inline bool long_ws_layout(int B, int T, int S, LongWs* w) {
    if (S > LONG_MAX_S) return false;
    const int L = 2 * S + 1;
    int K = 4, waves = 1;
    while (1024 * K < L) K <<= 1;
    while (64 * K * waves < L) waves <<= 1;
    w->K = K;
    w->waves = waves;
    w->total = ia_align_up((size_t)B * T * (size_t)(64 * waves) * (size_t)(K / 4), 256);
    return true;
}

__device__ __forceinline__ int wg_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

template <int K> struct BpWord;
template <> struct BpWord<4> { using type = uint8_t; };
template <> struct BpWord<8> { using type = uint16_t; };
template <> struct BpWord<16> { using type = uint32_t; };

template <int K, int PF, bool LOGITS>
__global__ __launch_bounds__(1024) void ctc_viterbi_wg(const float* __restrict__ lp, const float* __restrict__ lse,
                                                       const int64_t* __restrict__ targets, const int64_t* __restrict__ in_lens,
                                                       const int64_t* __restrict__ tg_lens, int T, int ld, int V, int S, int blank,
                                                       int32_t* __restrict__ path, int32_t* __restrict__ spans,
                                                       float* __restrict__ score, typename BpWord<K>::type* __restrict__ BP) {
    using Word = typename BpWord<K>::type;
    constexpr int H = K / 2;       // token states of a lane: state s0 + 2h + 1 is token s0/2 + h
    constexpr int KSH = K == 4 ? 2 : (K == 8 ? 3 : 4);
    constexpr int BT = 16;         // backtrace: frames per window load
    constexpr int NL = ((BT * 2 - 2 + K - 1) / K + 1 + 3) / 4;   // words [s/K - ceil(30/K), s/K], four per register
    __shared__ float xw[2][16];
    __shared__ float fin[2];
    const int b = blockIdx.x;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & 63, wave = wg_uniform(tid >> 6);
    int64_t tb64 = in_lens[b], sb64 = tg_lens[b];
    const int Tb = wg_uniform((int)(tb64 < 0 ? 0 : (tb64 > T ? T : tb64)));   // lengths beyond the buffers are clamped, never followed
    const int Sb = wg_uniform((int)(sb64 < 0 ? 0 : (sb64 > S ? S : sb64)));
    const int L = 2 * Sb + 1;
    int32_t* pathb = path + (size_t)b * T;
    int32_t* spanb = spans + (size_t)b * S * 2;
    // frames beyond the utterance and tokens beyond the transcript: disjoint from everything written below
    for (int t = Tb + tid; t < T; t += nthr) pathb[t] = -1;
    for (int i = 2 * Sb + tid; i < 2 * S; i += nthr) spanb[i] = -1;
    if (tid == 0) fin[0] = fin[1] = IA_NEG_INF;

    Word* bpb = BP + (size_t)b * T * nthr;
    if (Tb > 0) {
        const int s0 = tid * K;
        const int nvalid = L - s0;           // states j < nvalid of this lane exist
        int lab[H];
        unsigned skipmask = 0;
#pragma unroll
        for (int h = 0; h < H; ++h) {
            const int i = (s0 >> 1) + h;
            int l = blank, other = -1;
            if (i < Sb) {
                l = (int)targets[(int64_t)b * S + i];
                l = l < 0 ? 0 : (l > V - 1 ? V - 1 : l);   // a label outside the vocabulary must not become an address
                if (i >= 1) {
                    other = (int)targets[(int64_t)b * S + i - 1];
                    other = other < 0 ? 0 : (other > V - 1 ? V - 1 : other);
                }
            }
            lab[h] = l;
            if (other >= 0 && other != l) skipmask |= 1u << h;
        }
        const float* lpb = lp + (size_t)b * T * ld;
        const float* lseb = LOGITS ? lse + (size_t)b * T : nullptr;
        float prev[K], q[PF][H], qb[PF];
        {
            float z = 0.f;
            if constexpr (LOGITS) z = lseb[0];
            const float v0 = lpb[blank] - z, v1 = lpb[lab[0]] - z;
#pragma unroll
            for (int j = 0; j < K; ++j) prev[j] = IA_NEG_INF;
            if (tid == 0) {
                prev[0] = v0;                     // L >= 1
                if (L > 1) prev[1] = v1;
            }
        }
        if (lane == 63) xw[0][wave] = prev[K - 1];
#pragma unroll
        for (int i = 0; i < PF; ++i) {
            int t = 1 + i;
            t = t > Tb - 1 ? Tb - 1 : t;
            float z = 0.f;
            if constexpr (LOGITS) z = lseb[t];
            qb[i] = lpb[(size_t)t * ld + blank] - z;
#pragma unroll
            for (int h = 0; h < H; ++h) q[i][h] = lpb[(size_t)t * ld + lab[h]] - z;
        }
        __syncthreads();
        for (int n = 1; n < Tb; n += PF) {
#pragma unroll
            for (int i = 0; i < PF; ++i) {
                const int t = n + i;
                if (t < Tb) {
                    float n1 = ia_wave_shr1(prev[K - 1], IA_NEG_INF);
                    if (lane == 0 && wave > 0) n1 = xw[(t - 1) & 1][wave - 1];
                    unsigned word = 0;
#pragma unroll
                    for (int j = K - 1; j >= 0; --j) {
                        const float a1 = (j >= 1) ? prev[j >= 1 ? j - 1 : 0] : n1;
                        // torch.max over [stay, s-1, s-2]: the first maximum wins, so a later candidate needs strictly more
                        float m = prev[j];
                        unsigned bp = 0;
                        if (a1 > m) { m = a1; bp = 1; }
                        if (j & 1) {
                            const float a2raw = (j >= 2) ? prev[j >= 2 ? j - 2 : 0] : n1;
                            const float a2 = ((skipmask >> (j >> 1)) & 1u) ? a2raw : IA_NEG_INF;
                            if (a2 > m) { m = a2; bp = 2; }
                        }
                        const float qq = (j & 1) ? q[i][j >> 1] : qb[i];
                        prev[j] = (j < nvalid) ? m + qq : IA_NEG_INF;
                        word |= bp << (2 * j);
                    }
                    bpb[(size_t)t * nthr + tid] = (Word)word;
                    if (lane == 63) xw[t & 1][wave] = prev[K - 1];
                    int tf = t + PF;
                    tf = tf > Tb - 1 ? Tb - 1 : tf;
                    float zf = 0.f;
                    if constexpr (LOGITS) zf = lseb[tf];
                    qb[i] = lpb[(size_t)tf * ld + blank] - zf;
#pragma unroll
                    for (int h = 0; h < H; ++h) q[i][h] = lpb[(size_t)tf * ld + lab[h]] - zf;
                    __syncthreads();   // the frame's one barrier: xw[t & 1] is complete, xw[(t-1) & 1] is free
                }
            }
        }
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if (s0 + j == L - 1) fin[0] = prev[j];
            if (s0 + j == L - 2) fin[1] = prev[j];
        }
    }
    __syncthreads();   // fin; and every backpointer word of the utterance is visible to the workgroup
    const float a = fin[0], c2 = fin[1];
    // argmax over [L-2, L-1]: the last token wins a tie with the trailing blank; L = 1 has state 0 only
    const bool take_token = L > 1 && c2 >= a;
    const float best_end = Tb > 0 ? (take_token ? c2 : a) : IA_NEG_INF;
    const int s_end = take_token ? L - 2 : L - 1;
    const bool feasible = best_end != IA_NEG_INF;
    if (tid == 0) score[b] = best_end;
    if (!feasible) {
        for (int t = tid; t < Tb; t += nthr) pathb[t] = -1;
        for (int i = tid; i < 2 * Sb; i += nthr) spanb[i] = -1;
        return;
    }

    if (wave == 0) {
        const int fi = lane >> 2, fw = lane & 3;   // this lane's frame and word of a window
        int s = wg_uniform(s_end);
        int mine = -1;   // state of frame (row base + lane) of the 64-frame row being filled
        for (int t = Tb - 1; t >= 1; t -= BT) {
            const int base = s >> KSH;
            unsigned w[NL];
#pragma unroll
            for (int r = 0; r < NL; ++r) {
                const int tt = t - fi, wi = base - fw - 4 * r;
                w[r] = (tt >= 1 && wi >= 0) ? (unsigned)bpb[(size_t)tt * nthr + wi] : 0u;
            }
#pragma unroll
            for (int i = 0; i < BT; ++i) {
                const int tt = t - i;
                if (tt >= 1) {
                    if (lane == (tt & 63)) mine = s;
                    if ((tt & 63) == 0) {   // row [tt, tt+64) is complete
                        if (tt + lane < Tb) pathb[tt + lane] = mine;
                    }
                    const int d = base - (s >> KSH);          // 0 .. ceil(30/K) < 4 NL
                    const int src = i * 4 + (d & 3);
                    unsigned word = 0;
#pragma unroll
                    for (int r = 0; r < NL; ++r)
                        if ((d >> 2) == r) word = (unsigned)__builtin_amdgcn_readlane((int)w[r], src);
                    s -= (int)((word >> (2 * (s & (K - 1)))) & 3u);
                    s = s < 0 ? 0 : s;   // (a finite path never gets here: the state stays a valid word / span index regardless)
                }
            }
        }
        if (lane == 0) mine = s;
        if (lane < Tb) pathb[lane] = mine;   // row [0, 64)
    }
    // spans from the path just written (by wave 0): first and last frame of every odd state
    __syncthreads();
    for (int t = tid; t < Tb; t += nthr) {
        const int st = pathb[t];
        if (st > 0 && st < L && (st & 1)) {
            const int before = t > 0 ? pathb[t - 1] : -1;
            const int after = t + 1 < Tb ? pathb[t + 1] : -1;
            if (before != st) spanb[2 * (st >> 1)] = t;
            if (after != st) spanb[2 * (st >> 1) + 1] = t;
        }
    }
}

template <int K>
void launch_viterbi_wg(int waves, const float* lp, int ld, const float* lse, const int64_t* targets, const int64_t* il,
                       const int64_t* tl, int B, int T, int V, int S, int blank, int32_t* path, int32_t* spans, float* score, void* ws,
                       hipStream_t st) {
    constexpr int PF = 4;
    using Word = typename BpWord<K>::type;
    if (lse)
        hipLaunchKernelGGL((ctc_viterbi_wg<K, PF, true>), dim3(B), dim3(64 * waves), 0, st, lp, lse, targets, il, tl, T, ld, V, S,
                           blank, path, spans, score, (Word*)ws);
    else
        hipLaunchKernelGGL((ctc_viterbi_wg<K, PF, false>), dim3(B), dim3(64 * waves), 0, st, lp, lse, targets, il, tl, T, ld, V, S,
                           blank, path, spans, score, (Word*)ws);
}
}  // namespace

extern "C" int ia_ctc_align_long_max_targets(void) { return LONG_MAX_S; }

extern "C" size_t ia_ctc_align_long_workspace_bytes(int B, int T, int S) {
    LongWs w;
    if (B <= 0 || T <= 0 || S < 0 || !long_ws_layout(B, T, S, &w)) return 0;
    return w.total;
}

extern "C" int ia_ctc_align_long(const float* lp, int ld, const float* lse, const int64_t* targets, const int64_t* input_lens,
                                 const int64_t* target_lens, int B, int T, int V, int S, int blank, int32_t* path, int32_t* spans,
                                 float* score, void* workspace, size_t workspace_bytes, ia_stream_t stream) {
    if (!lp || !input_lens || !target_lens || !path || !score || B <= 0 || T <= 0 || V <= 0 || S < 0 || ld < V)
        return IA_INVALID_VALUE;
    if (S > 0 && (!targets || !spans)) return IA_INVALID_VALUE;
    if (blank < 0 || blank >= V) return IA_INVALID_VALUE;
    LongWs w;
    if (!long_ws_layout(B, T, S, &w)) return IA_UNSUPPORTED;
    if (!workspace || !ia_is_aligned(workspace, 256)) return IA_INVALID_VALUE;
    if (workspace_bytes < w.total) return IA_WORKSPACE_TOO_SMALL;
    hipStream_t st = (hipStream_t)stream;
    switch (w.K) {
        case 4: launch_viterbi_wg<4>(w.waves, lp, ld, lse, targets, input_lens, target_lens, B, T, V, S, blank, path, spans, score, workspace, st); break;
        case 8: launch_viterbi_wg<8>(w.waves, lp, ld, lse, targets, input_lens, target_lens, B, T, V, S, blank, path, spans, score, workspace, st); break;
        default: launch_viterbi_wg<16>(w.waves, lp, ld, lse, targets, input_lens, target_lens, B, T, V, S, blank, path, spans, score, workspace, st); break;
    }
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}
