// CTC prefix beam search for gfx950: the sum-product sibling of ctc_viterbi (csrc/ctc_align.hip).  The algorithm of Hannun et al.
// 2014 (arXiv:1408.2873) / Graves' prefix search in log space; the definition is the one in include/indicasr.h.
//
//   ctc_prefix_beam : one persistent workgroup (4 waves) per utterance, the whole search in one launch.
//     rows      a frame's V log-probs (x - lse) live in an LDS ring of PF frames; frame t + PF - 1 is loaded into registers at the
//               top of frame t and stored to the ring at its bottom.
//     beam      <= W slots in LDS: trie node, its parent node, last label, length, p = pb (+) pnb, pb, pnb -- the three RELATIVE to
//               the best score of the previous frame; the sum of those bests is carried in fp64 by one lane, so a long utterance
//               decides on differences of O(1) numbers.
//     frame     A  lane j < n: the stay of slot j; if the parent prefix of j is in the beam (slot i), the extension (i, last_j)
//                  denotes the same prefix: its term is folded into j's stay and bit i of dead[last_j] removes it from B.
//               B  thread `tid` owns the tokens c = tid, tid + 256, ... of every slot.  A candidate is the 64-bit key
//                  (orderable score, ~id).  The beam is kept in descending order of p, so the extensions p_i + lp[c] of one
//                  token descend with the slot: a thread offers the first slot of each of its tokens that is still to come.
//                  W rounds of "largest offered key" (DPP in the wave, one LDS word per wave, one barrier per round); only the
//                  winner's owner moves on.  The winners leave in beam order, so no sort follows.
//               C  lane r < m builds slot r of the new beam; an extension looks its (parent node, token) up in the utterance's
//                  open-addressing table and inserts node 1 + t W + r if it is new: prefix identity is the node id.
//     end       lane r walks the parent links of hypothesis r backwards into tokens[b, r, :len]; everybody pads.
//   No float atomics: the only atomics are the integer OR on dead[] / ends[] and the compare-and-swap of the table, neither of which
//   reaches a score, so two launches agree bit for bit.
#include "ctc_beam.h"

namespace {

template <bool LOGITS>
__global__ __launch_bounds__(BEAM_THREADS) void ctc_prefix_beam(const float* __restrict__ x, const float* __restrict__ lse,
                                                                const int64_t* __restrict__ in_lens, int T, int ld, int V, int blank,
                                                                int W, float min_logp, int32_t* __restrict__ tokens,
                                                                int32_t* __restrict__ lengths, float* __restrict__ scores,
                                                                unsigned char* __restrict__ ws, size_t per_utt, size_t nodes_bytes,
                                                                int table_size) {
    __shared__ float ring[BEAM_PF][BEAM_MAX_V];
    __shared__ unsigned dead[BEAM_MAX_V];       // bit i of dead[c]: the extension (i, c) is folded into a member's stay
    __shared__ unsigned ends[BEAM_MAX_V];       // bit i of ends[c]: slot i ends in c (its extension by c starts from pb: a list key)
    __shared__ int b_node[BEAM_MAX_W], b_par[BEAM_MAX_W], b_last[BEAM_MAX_W], b_len[BEAM_MAX_W], b_pi[BEAM_MAX_W];
    __shared__ float b_p[BEAM_MAX_W], b_pb[BEAM_MAX_W], b_pnb[BEAM_MAX_W], s_pb[BEAM_MAX_W], s_pnb[BEAM_MAX_W];
    __shared__ unsigned long long red[2][BEAM_WAVES], win[BEAM_MAX_W];
    __shared__ int b_n;
    __shared__ double offset;

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (IA_WAVE - 1), wave = tid / IA_WAVE;
    const int64_t tb64 = in_lens[b];
    const int Tb = (int)(tb64 < 0 ? 0 : (tb64 > T ? T : tb64));   // lengths beyond the buffer are clamped, never followed
    int2* nodes = (int2*)(ws + (size_t)b * per_utt);
    int* table = (int*)(ws + (size_t)b * per_utt + nodes_bytes);
    const int mask = table_size - 1;
    const float* xb = x + (size_t)b * T * ld;
    const float* lseb = LOGITS ? lse + (size_t)b * T : nullptr;

    for (int i = tid; i < table_size; i += BEAM_THREADS) table[i] = -1;
    for (int c = tid; c < BEAM_MAX_V; c += BEAM_THREADS) dead[c] = ends[c] = 0u;
    if (tid == 0) {
        nodes[0] = make_int2(-1, -1);
        b_node[0] = 0; b_par[0] = -1; b_last[0] = -1; b_len[0] = 0; b_p[0] = 0.f; b_pb[0] = 0.f; b_pnb[0] = IA_NEG_INF;
        b_n = 1;
        offset = 0.0;
    }
    for (int f = 0; f < BEAM_PF - 1 && f < Tb; ++f) {
        const float z = LOGITS ? lseb[f] : 0.f;
        for (int c = tid; c < V; c += BEAM_THREADS) ring[f][c] = xb[(size_t)f * ld + c] - z;
    }
    __syncthreads();

    for (int t = 0; t < Tb; ++t) {
        const int n = b_n;
        const float* lp = ring[t % BEAM_PF];
        const int tf = t + BEAM_PF - 1;
        float pre[BEAM_TOK];
        if (tf < Tb) {
            const float z = LOGITS ? lseb[tf] : 0.f;
#pragma unroll
            for (int k = 0; k < BEAM_TOK; ++k) {
                const int c = tid + k * BEAM_THREADS;
                pre[k] = c < V ? xb[(size_t)tf * ld + c] - z : 0.f;
            }
        }

        // ---- A: lane j < n: the stay of slot j, with the extension that denotes the same prefix folded in
        int my_dead = -1, my_end = -1;
        unsigned long long list_key = 0ull;      // the one candidate this thread owns that is no plain extension
        if (tid < n) {
            const int j = tid, e = b_last[j];
            const float p = b_p[j];
            const float spb = p + lp[blank];
            float spnb = e >= 0 ? b_pnb[j] + lp[e] : IA_NEG_INF;
            int id = j * V + blank, pi = -1;
            if (e >= 0) {
                atomicOr(&ends[e], 1u << j);
                my_end = e;
                const int par = b_par[j];
                for (int i = 0; i < n; ++i) pi = b_node[i] == par ? i : pi;
                if (pi >= 0 && !(lp[e] < min_logp)) {
                    const float base = b_last[pi] == e ? b_pb[pi] : b_p[pi];
                    spnb = ia_lse2(spnb, base + lp[e]);
                    id = min(id, pi * V + e);
                    atomicOr(&dead[e], 1u << pi);
                    my_dead = e;
                } else {
                    pi = -1;
                }
            }
            b_pi[j] = pi;
            s_pb[j] = spb; s_pnb[j] = spnb;
            list_key = beam_key(ia_lse2(spb, spnb), id);
        }
        __syncthreads();

        // ---- B: the m <= W largest keys, in order.  The beam is in descending order of p, and rounding is monotone, so the
        // plain extensions of one token, p_i + lp[c], descend with the slot (ties: the smaller id first): per token a mask of
        // the slots still to come, the lowest of which is that token's candidate.  The extensions that start from pb instead
        // (slot i ends in c) stand outside that order: they are list keys, like the stays.
        if (tid >= n && tid < 2 * n) {
            const int i = tid - n, e = b_last[i];
            if (e >= 0 && !(lp[e] < min_logp) && !((dead[e] >> i) & 1u)) list_key = beam_key(b_pb[i] + lp[e], i * V + e);
        }
        unsigned avail[BEAM_TOK];
        unsigned long long tok_key[BEAM_TOK];
        const unsigned all = n >= 32 ? 0xffffffffu : (1u << n) - 1u;
        auto candidate = [&](int k) {
            if (avail[k] == 0u) return 0ull;
            const int c = tid + k * BEAM_THREADS, i = __ffs((int)avail[k]) - 1;
            return beam_key(b_p[i] + lp[c], i * V + c);
        };
        unsigned long long mine = list_key;
#pragma unroll
        for (int k = 0; k < BEAM_TOK; ++k) {
            const int c = tid + k * BEAM_THREADS;
            avail[k] = (c < V && c != blank && !(lp[c] < min_logp)) ? all & ~dead[c] & ~ends[c] : 0u;
            tok_key[k] = candidate(k);
            mine = tok_key[k] > mine ? tok_key[k] : mine;
        }
        int m = 0;
        for (int r = 0; r < W; ++r) {
            const unsigned long long wv = beam_wave_max(mine);
            if (lane == 0) red[r & 1][wave] = wv;
            __syncthreads();
            unsigned long long winner = red[r & 1][0];
#pragma unroll
            for (int w = 1; w < BEAM_WAVES; ++w) winner = red[r & 1][w] > winner ? red[r & 1][w] : winner;
            if (winner == 0ull) break;       // fewer than W candidates (the same for every thread)
            if (tid == 0) win[r] = winner;
            ++m;
            if (mine == winner) {            // the owner alone moves on to its next candidate
                if (list_key == winner) list_key = 0ull;
                mine = list_key;
#pragma unroll
                for (int k = 0; k < BEAM_TOK; ++k) {
                    if (tok_key[k] == winner) {
                        avail[k] &= avail[k] - 1u;
                        tok_key[k] = candidate(k);
                    }
                    mine = tok_key[k] > mine ? tok_key[k] : mine;
                }
            }
        }
        __syncthreads();

        // ---- C: the new beam
        const float best = beam_unord((uint32_t)(win[0] >> 32));
        const float shift = best > IA_NEG_INF ? best : 0.f;
        int n_node = 0, n_par = -1, n_last = -1, n_len = 0;
        float n_p = IA_NEG_INF, n_pb = IA_NEG_INF, n_pnb = IA_NEG_INF;
        if (tid < m) {
            const unsigned long long key = win[tid];
            const int id = (int)(0xffffffffu - (uint32_t)(key & 0xffffffffu));
            const int i = id / V, c = id - i * V;
            // p of the next frame IS the score the beam was ordered by (minus the frame's best): B relies on that order
            n_p = beam_unord((uint32_t)(key >> 32)) - shift;
            int stay = c == blank ? i : -1;
            if (c != blank && ((dead[c] >> i) & 1u)) {          // the folded candidate under the extension's id
                for (int j = 0; j < n; ++j) stay = (b_pi[j] == i && b_last[j] == c) ? j : stay;
            }
            if (stay >= 0) {
                n_node = b_node[stay]; n_par = b_par[stay]; n_last = b_last[stay]; n_len = b_len[stay];
                n_pb = s_pb[stay] - shift; n_pnb = s_pnb[stay] - shift;
            } else {
                const int pnode = b_node[i];
                const int first_new = 1 + t * W, newid = first_new + tid;
                int found = -1;
                unsigned h = beam_hash(pnode, c) & mask;
                for (int probe = 0; probe < table_size && found < 0; ++probe) {
                    int e = beam_load(&table[h]);
                    if (e == -1) {
                        e = atomicCAS(&table[h], -1, newid);
                        if (e == -1) {
                            nodes[newid] = make_int2(pnode, c);
                            found = newid;
                            break;
                        }
                    }
                    if (e >= 0 && e < first_new) {               // a node of an earlier frame: its record is complete
                        const int2 nd = beam_load_node(&nodes[e]);
                        if (nd.x == pnode && nd.y == c) found = e;
                    }
                    h = (h + 1) & mask;
                }
                n_node = found < 0 ? 0 : found;                  // (never: the table is at most half full)
                n_par = pnode; n_last = c; n_len = min(b_len[i] + 1, T);
                n_pnb = n_p;
            }
        }
        __syncthreads();
        if (tid < m) {
            b_node[tid] = n_node; b_par[tid] = n_par; b_last[tid] = n_last; b_len[tid] = n_len;
            b_p[tid] = n_p; b_pb[tid] = n_pb; b_pnb[tid] = n_pnb;
        }
        if (my_dead >= 0) dead[my_dead] = 0u;
        if (my_end >= 0) ends[my_end] = 0u;
        if (tid == 0) {
            b_n = m;
            offset += (double)shift;
        }
        if (tf < Tb) {
#pragma unroll
            for (int k = 0; k < BEAM_TOK; ++k) {
                const int c = tid + k * BEAM_THREADS;
                if (c < V) ring[tf % BEAM_PF][c] = pre[k];
            }
        }
        __syncthreads();
    }

    // ---- the hypotheses: the beam is in order already
    const int n = b_n;
    int32_t* tokb = tokens + (size_t)b * W * T;
    for (int idx = tid; idx < W * T; idx += BEAM_THREADS) {
        const int r = idx / T, pos = idx - r * T;
        const int len = r < n ? b_len[r] : 0;
        if (pos >= len) tokb[idx] = -1;
    }
    if (tid < W) {
        const int r = tid;
        if (r < n) {
            lengths[(size_t)b * W + r] = b_len[r];
            scores[(size_t)b * W + r] = (float)(offset + (double)b_p[r]);
            int node = b_node[r], pos = b_len[r] - 1;
            while (node > 0 && pos >= 0) {
                const int2 nd = beam_load_node(&nodes[node]);
                tokb[(size_t)r * T + pos] = nd.y;
                --pos;
                node = nd.x;
            }
        } else {
            lengths[(size_t)b * W + r] = -1;
            scores[(size_t)b * W + r] = IA_NEG_INF;
        }
    }
}
}  // namespace

extern "C" int ia_ctc_beam_max_width(void) { return BEAM_MAX_W; }

extern "C" size_t ia_ctc_beam_workspace_bytes(int B, int T, int V, int W) {
    BeamWs w;
    if (B <= 0 || T <= 0 || V <= 0 || !beam_ws_layout(B, T, V, W, &w)) return 0;
    return w.total;
}

extern "C" int ia_ctc_beam_search(const float* x, const float* lse, const int64_t* in_lens, int B, int T, int ld, int V, int blank,
                                  int W, float token_min_logp, int32_t* tokens, int32_t* lengths, float* scores, void* workspace,
                                  size_t workspace_bytes, ia_stream_t stream) {
    if (!x || !in_lens || !tokens || !lengths || !scores || B <= 0 || T <= 0 || V <= 0 || ld < V || W < 1) return IA_INVALID_VALUE;
    if (blank < 0 || blank >= V || token_min_logp != token_min_logp) return IA_INVALID_VALUE;
    if (!ia_is_aligned(x, 4) || (lse && !ia_is_aligned(lse, 4)) || !ia_is_aligned(in_lens, 8) || !ia_is_aligned(tokens, 4) ||
        !ia_is_aligned(lengths, 4) || !ia_is_aligned(scores, 4))
        return IA_INVALID_VALUE;
    BeamWs w;
    if (!beam_ws_layout(B, T, V, W, &w)) return IA_UNSUPPORTED;
    if (!workspace || !ia_is_aligned(workspace, 256)) return IA_INVALID_VALUE;
    if (workspace_bytes < w.total) return IA_WORKSPACE_TOO_SMALL;
    hipStream_t st = (hipStream_t)stream;
    if (lse)
        hipLaunchKernelGGL((ctc_prefix_beam<true>), dim3(B), dim3(BEAM_THREADS), 0, st, x, lse, in_lens, T, ld, V, blank, W,
                           token_min_logp, tokens, lengths, scores, (unsigned char*)workspace, w.per_utt, w.nodes_bytes, w.table);
    else
        hipLaunchKernelGGL((ctc_prefix_beam<false>), dim3(B), dim3(BEAM_THREADS), 0, st, x, lse, in_lens, T, ld, V, blank, W,
                           token_min_logp, tokens, lengths, scores, (unsigned char*)workspace, w.per_utt, w.nodes_bytes, w.table);
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}
