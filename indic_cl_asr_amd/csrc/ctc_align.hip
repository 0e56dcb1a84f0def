// CTC forced alignment for gfx950: the max-plus twin of ctc_alpha_beta (csrc/ctc.hip) with backpointers and the backtrace in
// the same launch.  Semantics: NeMo forced aligner's viterbi_decoding (tools/nemo_forced_aligner/utils/viterbi_decoding.py:19-136)
// run on one utterance alone, including torch.max's first-maximum tie-break over [stay, s-1, s-2] and the final
// argmax over [L-2, L-1].
//
//   ctc_viterbi : one wave per utterance.  Lane owns K consecutive extended-label states (L = 2S+1 <= 64*K, K in {1,2,4,8});
//                 the s-1 / s-2 neighbours cross lanes by DPP wave shifts; the K gathers of a frame are prefetched PF frames
//                 ahead.  Per frame the lane packs its K 2-bit backpointers into one 16-bit word: a frame is 64 words = 128
//                 bytes of workspace, written coalesced and never waited for.
//                 Backtrace: the 64 words of a frame do not depend on the path, so the wave loads them BT frames ahead (one
//                 word per lane); the dependent chain per frame is v_readlane(word, s / K) -> bit extract -> subtract, all on
//                 the scalar unit.  The state of frame t is parked in lane t % 64 and the path leaves in 64-frame rows.
//                 Spans: a last pass over the path just written, one frame per lane.
#include "ia_common.h"

namespace {

constexpr int ALIGN_MAX_S = 255;

struct AlignWs { int K; size_t total; };

static inline bool align_ws_layout(int B, int T, int S, AlignWs* w) {
    const int L = 2 * S + 1;
    int K = 1;
    while (64 * K < L) K <<= 1;
    if (K > 8) return false;
    w->K = K;
    w->total = ia_align_up((size_t)B * T * 64 * sizeof(uint16_t), 256);
    return true;
}

__device__ __forceinline__ int wave_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

template <int K, int PF, bool LOGITS>
__global__ __launch_bounds__(64) void ctc_viterbi(const float* __restrict__ lp, const float* __restrict__ lse,
                                                  const int64_t* __restrict__ targets, const int64_t* __restrict__ in_lens,
                                                  const int64_t* __restrict__ tg_lens, int T, int ld, int V, int S, int blank,
                                                  int32_t* __restrict__ path, int32_t* __restrict__ spans,
                                                  float* __restrict__ score, uint16_t* __restrict__ BP) {
    constexpr int BT = 8;      // backtrace: frames of backpointer words in flight
    constexpr int KSH = K == 1 ? 0 : (K == 2 ? 1 : (K == 4 ? 2 : 3));
    const int b = blockIdx.x;
    const int lane = threadIdx.x;
    int64_t tb64 = in_lens[b], sb64 = tg_lens[b];
    const int Tb = wave_uniform((int)(tb64 < 0 ? 0 : (tb64 > T ? T : tb64)));   // lengths beyond the buffers are clamped, never followed
    const int Sb = wave_uniform((int)(sb64 < 0 ? 0 : (sb64 > S ? S : sb64)));
    const int L = 2 * Sb + 1;
    int32_t* pathb = path + (size_t)b * T;
    int32_t* spanb = spans + (size_t)b * S * 2;
    // frames beyond the utterance and tokens beyond the transcript: disjoint from everything written below
    for (int t = Tb + lane; t < T; t += 64) pathb[t] = -1;
    for (int i = 2 * Sb + lane; i < 2 * S; i += 64) spanb[i] = -1;

    float best_end = IA_NEG_INF;
    int s_end = 0;
    if (Tb > 0) {
        const int s0 = lane * K;
        int lab[K];
        bool skip[K];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const int s = s0 + j;
            int l = (s < L && (s & 1)) ? (int)targets[(int64_t)b * S + (s >> 1)] : blank;
            l = l < 0 ? 0 : (l > V - 1 ? V - 1 : l);   // a label outside the vocabulary must not become an address
            lab[j] = l;
            int other = -1;
            if (s >= 3 && s < L && (s & 1)) {
                other = (int)targets[(int64_t)b * S + ((s - 2) >> 1)];
                other = other < 0 ? 0 : (other > V - 1 ? V - 1 : other);
            }
            skip[j] = other >= 0 && other != l;
        }
        const float* lpb = lp + (size_t)b * T * ld;
        const float* lseb = LOGITS ? lse + (size_t)b * T : nullptr;
        uint16_t* bpb = BP + (size_t)b * T * 64 + lane;
        float prev[K], cur[K], q[PF][K];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const int s = s0 + j;
            float v0 = lpb[lab[j]];
            if constexpr (LOGITS) v0 -= lseb[0];
            prev[j] = (s < 2 && s < L) ? v0 : IA_NEG_INF;
        }
#pragma unroll
        for (int i = 0; i < PF; ++i) {
            int t = 1 + i;
            t = t > Tb - 1 ? Tb - 1 : t;
            float z = 0.f;
            if constexpr (LOGITS) z = lseb[t];
#pragma unroll
            for (int j = 0; j < K; ++j) q[i][j] = lpb[(size_t)t * ld + lab[j]] - z;
        }
        for (int n = 1; n < Tb; n += PF) {
#pragma unroll
            for (int i = 0; i < PF; ++i) {
                const int t = n + i;
                if (t < Tb) {
                    const float n1 = ia_wave_shr1(prev[K - 1], IA_NEG_INF);
                    float n2;
                    if constexpr (K >= 2) n2 = ia_wave_shr1(prev[K - 2], IA_NEG_INF);
                    else n2 = ia_wave_shr1(n1, IA_NEG_INF);
                    unsigned word = 0;
#pragma unroll
                    for (int j = 0; j < K; ++j) {
                        const int s = s0 + j;
                        const float a1 = (j >= 1) ? prev[j >= 1 ? j - 1 : 0] : n1;
                        const float a2raw = (j >= 2) ? prev[j >= 2 ? j - 2 : 0] : (j == 1 ? n1 : n2);
                        const float a2 = skip[j] ? a2raw : IA_NEG_INF;
                        // torch.max over [stay, s-1, s-2]: the first maximum wins, so a later candidate needs strictly more
                        float m = prev[j];
                        unsigned bp = 0;
                        if (a1 > m) { m = a1; bp = 1; }
                        if (a2 > m) { m = a2; bp = 2; }
                        cur[j] = (s < L) ? m + q[i][j] : IA_NEG_INF;
                        word |= bp << (2 * j);
                    }
                    bpb[(size_t)t * 64] = (uint16_t)word;
#pragma unroll
                    for (int j = 0; j < K; ++j) prev[j] = cur[j];
                    int tf = t + PF;
                    tf = tf > Tb - 1 ? Tb - 1 : tf;
                    float zf = 0.f;
                    if constexpr (LOGITS) zf = lseb[tf];
#pragma unroll
                    for (int j = 0; j < K; ++j) q[i][j] = lpb[(size_t)tf * ld + lab[j]] - zf;
                }
            }
        }
        float a = IA_NEG_INF, c2 = IA_NEG_INF;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if (s0 + j == L - 1) a = prev[j];
            if (s0 + j == L - 2) c2 = prev[j];
        }
        a = ia_wave_max_dpp(a);     // one lane holds the candidate, the rest -inf
        c2 = ia_wave_max_dpp(c2);
        // argmax over [L-2, L-1]: the last token wins a tie with the trailing blank; L = 1 has state 0 only
        const bool take_token = L > 1 && c2 >= a;
        best_end = take_token ? c2 : a;
        s_end = take_token ? L - 2 : L - 1;
    }
    const bool feasible = best_end != IA_NEG_INF;
    if (lane == 0) score[b] = best_end;
    if (!feasible) {
        for (int t = lane; t < Tb; t += 64) pathb[t] = -1;
        for (int i = lane; i < 2 * Sb; i += 64) spanb[i] = -1;
        return;
    }
    // the backpointer words were written by other lanes of this wave: make them visible before they are read back
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");

    const uint16_t* bpr = BP + (size_t)b * T * 64 + lane;
    int s = wave_uniform(s_end);
    unsigned nxt[BT], w[BT];
#pragma unroll
    for (int i = 0; i < BT; ++i) {
        const int tt = Tb - 1 - i;
        nxt[i] = tt >= 1 ? bpr[(size_t)tt * 64] : 0;
    }
    int mine = -1;   // state of frame (row base + lane) of the 64-frame row being filled
    for (int t = Tb - 1; t >= 1; t -= BT) {
#pragma unroll
        for (int i = 0; i < BT; ++i) w[i] = nxt[i];
#pragma unroll
        for (int i = 0; i < BT; ++i) {
            const int tt = t - BT - i;
            nxt[i] = tt >= 1 ? bpr[(size_t)tt * 64] : 0;
        }
#pragma unroll
        for (int i = 0; i < BT; ++i) {
            const int tt = t - i;
            if (tt >= 1) {
                if (lane == (tt & 63)) mine = s;
                if ((tt & 63) == 0) {   // row [tt, tt+64) is complete
                    if (tt + lane < Tb) pathb[tt + lane] = mine;
                }
                const unsigned word = (unsigned)__builtin_amdgcn_readlane((int)w[i], s >> KSH);
                s -= (int)((word >> (2 * (s & (K - 1)))) & 3u);
                s = s < 0 ? 0 : s;   // (a finite path never gets here: the state stays a valid lane / span index regardless)
            }
        }
    }
    if (lane == 0) mine = s;
    if (lane < Tb) pathb[lane] = mine;   // row [0, 64)

    // spans from the path just written (by other lanes): first and last frame of every odd state
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    for (int t = lane; t < Tb; t += 64) {
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
void launch_viterbi(const float* lp, int ld, const float* lse, const int64_t* targets, const int64_t* il, const int64_t* tl, int B,
                    int T, int V, int S, int blank, int32_t* path, int32_t* spans, float* score, void* ws, hipStream_t st) {
    constexpr int PF = (K >= 8) ? 2 : 4;   // as the loss
    if (lse)
        hipLaunchKernelGGL((ctc_viterbi<K, PF, true>), dim3(B), dim3(64), 0, st, lp, lse, targets, il, tl, T, ld, V, S, blank, path,
                           spans, score, (uint16_t*)ws);
    else
        hipLaunchKernelGGL((ctc_viterbi<K, PF, false>), dim3(B), dim3(64), 0, st, lp, lse, targets, il, tl, T, ld, V, S, blank, path,
                           spans, score, (uint16_t*)ws);
}
}  // namespace

extern "C" int ia_ctc_align_max_targets(void) { return ALIGN_MAX_S; }

extern "C" size_t ia_ctc_align_workspace_bytes(int B, int T, int S) {
    AlignWs w;
    if (B <= 0 || T <= 0 || S < 0 || !align_ws_layout(B, T, S, &w)) return 0;
    return w.total;
}

extern "C" int ia_ctc_align(const float* lp, int ld, const float* lse, const int64_t* targets, const int64_t* input_lens,
                            const int64_t* target_lens, int B, int T, int V, int S, int blank, int32_t* path, int32_t* spans,
                            float* score, void* workspace, size_t workspace_bytes, ia_stream_t stream) {
    if (!lp || !input_lens || !target_lens || !path || !score || B <= 0 || T <= 0 || V <= 0 || S < 0 || ld < V)
        return IA_INVALID_VALUE;
    if (S > 0 && (!targets || !spans)) return IA_INVALID_VALUE;
    if (blank < 0 || blank >= V) return IA_INVALID_VALUE;
    AlignWs w;
    if (!align_ws_layout(B, T, S, &w)) return IA_UNSUPPORTED;
    if (!workspace || !ia_is_aligned(workspace, 256)) return IA_INVALID_VALUE;
    if (workspace_bytes < w.total) return IA_WORKSPACE_TOO_SMALL;
    hipStream_t st = (hipStream_t)stream;
    switch (w.K) {
        case 1: launch_viterbi<1>(lp, ld, lse, targets, input_lens, target_lens, B, T, V, S, blank, path, spans, score, workspace, st); break;
        case 2: launch_viterbi<2>(lp, ld, lse, targets, input_lens, target_lens, B, T, V, S, blank, path, spans, score, workspace, st); break;
        case 4: launch_viterbi<4>(lp, ld, lse, targets, input_lens, target_lens, B, T, V, S, blank, path, spans, score, workspace, st); break;
        default: launch_viterbi<8>(lp, ld, lse, targets, input_lens, target_lens, B, T, V, S, blank, path, spans, score, workspace, st); break;
    }
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}
