// CTC prefix beam search with n-gram LM shallow fusion for gfx950: csrc/ctc_beam.hip with ONE rule changed -- an extension of the
// member l by c != blank carries alpha ln P_LM(c | h(l)) + beta (stays carry none).  The definition and the image of the back-off
// model (ia_ngram_lm) are in include/indicasr.h.
//
//   ctc_prefix_beam_lm : one persistent workgroup (4 waves) per utterance, the whole search in one launch; rows / beam / trie / end
//   as in ctc_prefix_beam.  What differs:
//     state     every beam slot carries its LM state (the longest suffix of <s> l that is a context of the model) and the index of
//               its ROW in a pool of 2 W rows per utterance: row[c] = alpha lm(state, c) + beta and next[c] = the state after c,
//               for all V classes.  The values sit in LDS where 2 W V floats fit into 128 KB (LDS_ROWS), else in the workspace
//               (L2-resident), as next[] always does (it is read once per new member).  A stay inherits state and row; an
//               extension reads its state from its parent's next[] and takes a row that no stay of the new beam holds (at
//               most W are held, so W are free).
//     build     rows are built only for the new members of a frame: lane r walks the back-off chain of its state once (at most
//               order - 1 steps: the arc ranges and the back-off sums above them go to LDS); every thread fills the new rows
//               from the unigram values of the classes it owns (registers: stores only); then one pass per chain level,
//               shortest context first, a wave per row, overwrites the entries of that context's arcs.  A barrier separates
//               the levels, so the longest context that holds c wins, whatever the timing.
//     frame  A  the extension folded into a member's stay carries its LM term.
//            B  with the LM term the extensions of a token no longer descend with the slot, so a thread keeps, per token it owns,
//               the LARGEST key over the slots still available (a mask), and after a win the owner alone drops the winner's slot
//               and scans that token's slots again.  Same keys, same tie rule, same W rounds as ctc_prefix_beam; "slot i ends
//               in c" (start from pb) needs no list of its own here, every (slot, token) is looked at singly.
//   Every walk is bounded and every index read from the image is clamped to its array: a corrupt image gives wrong scores, not
//   a wild access.  No float atomics; the integer ones (dead[], the chain depth, the table) reach no score.
#include "ctc_beam.h"

namespace {

constexpr int LM_MAX_ORDER = 8;
constexpr size_t LM_LDS_ROWS_MAX = 128 * 1024;    // dynamic LDS for the rows, beside 26 KB of static LDS, of the CU's 160 KB

struct BeamLmWs { BeamWs base; size_t rows_bytes, per_utt, total; };

static inline bool beam_lm_ws_layout(int B, int T, int V, int W, BeamLmWs* w) {
    if (!beam_ws_layout(B, T, V, W, &w->base)) return false;
    w->rows_bytes = ia_align_up((size_t)2 * W * V * sizeof(float), 256);      // the values; as many bytes again for next[]
    w->per_utt = w->base.per_utt + 2 * w->rows_bytes;
    w->total = w->per_utt * (size_t)B;
    return true;
}

__device__ __forceinline__ float beam_load_f(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int beam_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <bool LOGITS, bool LDS_ROWS>
__global__ __launch_bounds__(BEAM_THREADS) void ctc_prefix_beam_lm(const float* __restrict__ x, const float* __restrict__ lse,
                                                                   const int64_t* __restrict__ in_lens, int T, int ld, int V,
                                                                   int blank, int W, float min_logp, ia_ngram_lm lm, float alpha,
                                                                   float beta, int32_t* __restrict__ tokens,
                                                                   int32_t* __restrict__ lengths, float* __restrict__ scores,
                                                                   unsigned char* ws, size_t per_utt, size_t nodes_bytes,
                                                                   size_t base_bytes, size_t rows_bytes, int table_size) {
    extern __shared__ __attribute__((aligned(16))) float lds_rows[];     // LDS_ROWS: the values of the 2 W rows
    __shared__ float ring[BEAM_PF][BEAM_MAX_V];
    __shared__ unsigned dead[BEAM_MAX_V];       // bit i of dead[c]: the extension (i, c) is folded into a member's stay
    __shared__ int b_node[BEAM_MAX_W], b_par[BEAM_MAX_W], b_last[BEAM_MAX_W], b_len[BEAM_MAX_W], b_pi[BEAM_MAX_W];
    __shared__ int b_state[BEAM_MAX_W], b_row[BEAM_MAX_W], b_new[BEAM_MAX_W];
    __shared__ float b_p[BEAM_MAX_W], b_pb[BEAM_MAX_W], b_pnb[BEAM_MAX_W], s_pb[BEAM_MAX_W], s_pnb[BEAM_MAX_W];
    __shared__ int ch_a0[BEAM_MAX_W][LM_MAX_ORDER], ch_a1[BEAM_MAX_W][LM_MAX_ORDER];   // the arcs of a new member's back-off chain,
    __shared__ int ch_depth[BEAM_MAX_W], new_list[BEAM_MAX_W];                          // deepest first; the slots that are new
    __shared__ float ch_acc[BEAM_MAX_W][LM_MAX_ORDER], ch_root[BEAM_MAX_W];       // the back-off sum above each level / above the root
    __shared__ unsigned long long red[2][BEAM_WAVES], win[BEAM_MAX_W];
    __shared__ int b_n, s_maxd, s_nnew;
    __shared__ double offset;

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (IA_WAVE - 1), wave = tid / IA_WAVE;
    const int64_t tb64 = in_lens[b];
    const int Tb = (int)(tb64 < 0 ? 0 : (tb64 > T ? T : tb64));   // lengths beyond the buffer are clamped, never followed
    unsigned char* wsb = ws + (size_t)b * per_utt;
    int2* nodes = (int2*)wsb;
    int* table = (int*)(wsb + nodes_bytes);
    float* rows = LDS_ROWS ? lds_rows : (float*)(wsb + base_bytes);       // [2 W, V]
    auto row_at = [&](int slot, int c) {                          // alpha lm + beta of the member in `slot` for the class c
        const float* p = &rows[(size_t)b_row[slot] * V + c];
        return LDS_ROWS ? *p : beam_load_f(p);
    };
    int* rnext = (int*)(wsb + base_bytes + rows_bytes);           // [2 W, V]
    const int mask = table_size - 1;
    const float* xb = x + (size_t)b * T * ld;
    const float* lseb = LOGITS ? lse + (size_t)b * T : nullptr;
    const int last_state = lm.n_states - 1;
    const int chain_max = min(lm.order, LM_MAX_ORDER) - 1;
    float uni_v[BEAM_TOK];                                        // the unigram row of the classes this thread owns
    int uni_n[BEAM_TOK];
#pragma unroll
    for (int k = 0; k < BEAM_TOK; ++k) {
        const int c = tid + k * BEAM_THREADS;
        const bool known = c < V && c < lm.n_tokens;
        uni_v[k] = known ? lm.uni_logp[c] : lm.unk_logp;
        uni_n[k] = known ? beam_clamp(lm.uni_next[c], 0, last_state) : 0;
    }

    // the rows of the new members among slots 0 .. m-1 (b_new set, b_state and b_row in place); every thread calls it with the same m
    auto build_rows = [&](int m) {
        if (wave == 0) {
            const bool is_new = tid < m && b_new[tid];
            const unsigned long long news = __ballot(is_new);
            if (is_new) {
                int s = beam_clamp(b_state[tid], 0, last_state), d = 0;
                float acc = 0.f;
                for (int k = 0; k < chain_max && s > 0; ++k) {
                    const int a0 = beam_clamp(lm.states[3 * s + 1], 0, lm.n_arcs);
                    ch_a0[tid][d] = a0;
                    ch_a1[tid][d] = beam_clamp(lm.states[3 * s + 2], a0, lm.n_arcs);
                    ch_acc[tid][d] = acc;
                    acc += lm.backoff[s];
                    s = beam_clamp(lm.states[3 * s], 0, last_state);
                    ++d;
                }
                ch_depth[tid] = d;
                ch_root[tid] = acc;
                new_list[__popcll(news & ((1ull << lane) - 1ull))] = tid;
                atomicMax(&s_maxd, d);
            }
            if (lane == 0) s_nnew = __popcll(news);
        }
        __syncthreads();
        const int nnew = s_nnew, maxd = s_maxd;
        if (nnew == 0) return;                                    // nobody is new (the same for every thread)
        for (int q = 0; q < nnew; ++q) {                          // the dense fill: every thread its own classes, stores only
            const int r = new_list[q];
            float* row = rows + (size_t)b_row[r] * V;
            int* nxt = rnext + (size_t)b_row[r] * V;
            const float acc = ch_root[r];
#pragma unroll
            for (int k = 0; k < BEAM_TOK; ++k) {
                const int c = tid + k * BEAM_THREADS;
                if (c < V) {
                    row[c] = alpha * (acc + uni_v[k]) + beta;
                    nxt[c] = uni_n[k];
                }
            }
        }
        for (int lvl = 1; lvl <= maxd; ++lvl) {                   // shortest context first; the longest that holds c writes last
            __syncthreads();
            // a wave per new row, its (at most BEAM_MAX_W / BEAM_WAVES) rows together: all loads of the first 64 arcs, then the stores
            int a_tok[BEAM_MAX_W / BEAM_WAVES], a_next[BEAM_MAX_W / BEAM_WAVES];
            float a_val[BEAM_MAX_W / BEAM_WAVES];
#pragma unroll
            for (int j = 0; j < BEAM_MAX_W / BEAM_WAVES; ++j) {
                const int q = wave + j * BEAM_WAVES;
                a_tok[j] = -1;
                if (q < nnew) {
                    const int r = new_list[q], k = ch_depth[r] - lvl;
                    if (k >= 0) {
                        const int a = ch_a0[r][k] + lane;
                        if (a < ch_a1[r][k]) {
                            a_tok[j] = lm.arcs[2 * a];
                            a_next[j] = lm.arcs[2 * a + 1];
                            a_val[j] = alpha * (ch_acc[r][k] + lm.arc_logp[a]) + beta;
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < BEAM_MAX_W / BEAM_WAVES; ++j) {
                if (a_tok[j] >= 0 && a_tok[j] < V) {
                    const int r = new_list[wave + j * BEAM_WAVES];
                    rows[(size_t)b_row[r] * V + a_tok[j]] = a_val[j];
                    rnext[(size_t)b_row[r] * V + a_tok[j]] = beam_clamp(a_next[j], 0, last_state);
                }
            }
            for (int q = wave; q < nnew; q += BEAM_WAVES) {       // contexts with more than 64 arcs: the rest
                const int r = new_list[q], k = ch_depth[r] - lvl;
                if (k < 0) continue;
                const float acc = ch_acc[r][k];
                const int a1 = ch_a1[r][k];
                for (int a = ch_a0[r][k] + IA_WAVE + lane; a < a1; a += IA_WAVE) {
                    const int c = lm.arcs[2 * a];
                    if (c >= 0 && c < V) {
                        rows[(size_t)b_row[r] * V + c] = alpha * (acc + lm.arc_logp[a]) + beta;
                        rnext[(size_t)b_row[r] * V + c] = beam_clamp(lm.arcs[2 * a + 1], 0, last_state);
                    }
                }
            }
        }
        __syncthreads();
    };

    for (int i = tid; i < table_size; i += BEAM_THREADS) table[i] = -1;
    for (int c = tid; c < BEAM_MAX_V; c += BEAM_THREADS) dead[c] = 0u;
    if (tid == 0) {
        nodes[0] = make_int2(-1, -1);
        b_node[0] = 0; b_par[0] = -1; b_last[0] = -1; b_len[0] = 0; b_p[0] = 0.f; b_pb[0] = 0.f; b_pnb[0] = IA_NEG_INF;
        b_state[0] = lm.start; b_row[0] = 0; b_new[0] = 1;
        b_n = 1;
        s_maxd = -1;
        offset = 0.0;
    }
    for (int f = 0; f < BEAM_PF - 1 && f < Tb; ++f) {
        const float z = LOGITS ? lseb[f] : 0.f;
        for (int c = tid; c < V; c += BEAM_THREADS) ring[f][c] = xb[(size_t)f * ld + c] - z;
    }
    __syncthreads();
    if (Tb > 0) build_rows(1);

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

        // ---- A: lane j < n: the stay of slot j, with the extension that denotes the same prefix (LM term included) folded in
        int my_dead = -1;
        unsigned long long list_key = 0ull;      // the stay this thread owns
        if (tid < n) {
            const int j = tid, e = b_last[j];
            const float p = b_p[j];
            const float spb = p + lp[blank];
            float spnb = e >= 0 ? b_pnb[j] + lp[e] : IA_NEG_INF;
            int id = j * V + blank, pi = -1;
            if (e >= 0) {
                const int par = b_par[j];
                for (int i = 0; i < n; ++i) pi = b_node[i] == par ? i : pi;
                if (pi >= 0 && !(lp[e] < min_logp)) {
                    const float base = b_last[pi] == e ? b_pb[pi] : b_p[pi];
                    spnb = ia_lse2(spnb, (base + lp[e]) + row_at(pi, e));
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
        if (tid == 0) s_maxd = -1;
        __syncthreads();

        // ---- B: the m <= W largest keys, in order: per owned token the largest key over the slots still available
        unsigned avail[BEAM_TOK];
        unsigned long long tok_key[BEAM_TOK];
        const unsigned all = n >= 32 ? 0xffffffffu : (1u << n) - 1u;
        auto candidate = [&](int k) {            // the largest key of token k over the slots in avail[k]
            const int c = tid + k * BEAM_THREADS;
            const unsigned a = avail[k];
            unsigned long long best = 0ull;
            if (a == 0u) return best;            // (also every c >= V)
            const float l = lp[c];
#pragma unroll 4
            for (int i = 0; i < n; ++i) {        // every slot, the mask picks afterwards: the LDS reads of four slots go out together
                const float base = b_last[i] == c ? b_pb[i] : b_p[i];
                const unsigned long long key = beam_key((base + l) + row_at(i, c), i * V + c);
                best = (((a >> i) & 1u) && key > best) ? key : best;
            }
            return best;
        };
        unsigned long long mine = list_key;
#pragma unroll
        for (int k = 0; k < BEAM_TOK; ++k) {
            const int c = tid + k * BEAM_THREADS;
            avail[k] = (c < V && c != blank && !(lp[c] < min_logp)) ? all & ~dead[c] : 0u;
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
            if (mine == winner) {            // the owner alone moves on: without the winner's slot, that token's maximum again
                if (list_key == winner) list_key = 0ull;
                mine = list_key;
                const int wslot = (int)(0xffffffffu - (uint32_t)(winner & 0xffffffffu)) / V;
#pragma unroll
                for (int k = 0; k < BEAM_TOK; ++k) {
                    if (tok_key[k] == winner) {
                        avail[k] &= ~(1u << (wslot & 31));
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
        int n_node = 0, n_par = -1, n_last = -1, n_len = 0, n_state = 0, n_row = -1, n_new = 0;
        float n_p = IA_NEG_INF, n_pb = IA_NEG_INF, n_pnb = IA_NEG_INF;
        if (tid < m) {
            const unsigned long long key = win[tid];
            const int id = (int)(0xffffffffu - (uint32_t)(key & 0xffffffffu));
            const int i = id / V, c = id - i * V;
            n_p = beam_unord((uint32_t)(key >> 32)) - shift;
            int stay = c == blank ? i : -1;
            if (c != blank && ((dead[c] >> i) & 1u)) {          // the folded candidate under the extension's id
                for (int j = 0; j < n; ++j) stay = (b_pi[j] == i && b_last[j] == c) ? j : stay;
            }
            if (stay >= 0) {
                n_node = b_node[stay]; n_par = b_par[stay]; n_last = b_last[stay]; n_len = b_len[stay];
                n_state = b_state[stay]; n_row = b_row[stay];
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
                n_state = beam_clamp(beam_load(&rnext[(size_t)b_row[i] * V + c]), 0, last_state);
                n_new = 1;
            }
        }
        __syncthreads();
        if (tid < m) {
            b_node[tid] = n_node; b_par[tid] = n_par; b_last[tid] = n_last; b_len[tid] = n_len;
            b_p[tid] = n_p; b_pb[tid] = n_pb; b_pnb[tid] = n_pnb;
            b_state[tid] = n_state; b_row[tid] = n_row; b_new[tid] = n_new;
        }
        if (my_dead >= 0) dead[my_dead] = 0u;
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
        if (tid < m && n_new) {              // the rank-th row that no stay of the new beam holds (at most W of the 2 W are held)
            unsigned long long used = 0ull;
            int rank = 0;
            for (int j = 0; j < m; ++j) {
                if (!b_new[j]) used |= 1ull << (b_row[j] & 63);
                else if (j < tid) ++rank;
            }
            int row = 0;
            for (int q = 0; q < 2 * W; ++q) {
                if (!((used >> q) & 1ull)) {
                    if (rank == 0) { row = q; break; }
                    --rank;
                }
            }
            b_row[tid] = row;
        }
        if (t + 1 < Tb) build_rows(m);       // (a barrier precedes every read of b_row in there)
        else __syncthreads();
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

extern "C" int ia_ctc_beam_lm_max_order(void) { return LM_MAX_ORDER; }

extern "C" size_t ia_ctc_beam_lm_workspace_bytes(int B, int T, int V, int W) {
    BeamLmWs w;
    if (B <= 0 || T <= 0 || V <= 0 || !beam_lm_ws_layout(B, T, V, W, &w)) return 0;
    return w.total;
}

extern "C" int ia_ctc_beam_search_lm(const float* x, const float* lse, const int64_t* in_lens, int B, int T, int ld, int V, int blank,
                                     int W, float token_min_logp, const ia_ngram_lm* lm, float alpha, float beta, int32_t* tokens,
                                     int32_t* lengths, float* scores, void* workspace, size_t workspace_bytes, ia_stream_t stream) {
    if (!x || !in_lens || !tokens || !lengths || !scores || B <= 0 || T <= 0 || V <= 0 || ld < V || W < 1) return IA_INVALID_VALUE;
    if (blank < 0 || blank >= V || token_min_logp != token_min_logp) return IA_INVALID_VALUE;
    if (!ia_is_aligned(x, 4) || (lse && !ia_is_aligned(lse, 4)) || !ia_is_aligned(in_lens, 8) || !ia_is_aligned(tokens, 4) ||
        !ia_is_aligned(lengths, 4) || !ia_is_aligned(scores, 4))
        return IA_INVALID_VALUE;
    if (!lm || alpha != alpha || beta != beta) return IA_INVALID_VALUE;
    if (!lm->states || !lm->backoff || !lm->arcs || !lm->arc_logp || !lm->uni_logp || !lm->uni_next) return IA_INVALID_VALUE;
    if (!ia_is_aligned(lm->states, 4) || !ia_is_aligned(lm->backoff, 4) || !ia_is_aligned(lm->arcs, 4) ||
        !ia_is_aligned(lm->arc_logp, 4) || !ia_is_aligned(lm->uni_logp, 4) || !ia_is_aligned(lm->uni_next, 4))
        return IA_INVALID_VALUE;
    if (lm->order < 1 || lm->n_states < 1 || lm->n_arcs < 0 || lm->n_tokens < 1 || lm->start < 0 || lm->start >= lm->n_states ||
        lm->unk_logp != lm->unk_logp)
        return IA_INVALID_VALUE;
    if (lm->order == 1 && (lm->n_states != 1 || lm->n_arcs != 0)) return IA_INVALID_VALUE;     // a unigram model has the root alone
    if (lm->order > LM_MAX_ORDER) return IA_UNSUPPORTED;
    BeamLmWs w;
    if (!beam_lm_ws_layout(B, T, V, W, &w)) return IA_UNSUPPORTED;
    if (!workspace || !ia_is_aligned(workspace, 256)) return IA_INVALID_VALUE;
    if (workspace_bytes < w.total) return IA_WORKSPACE_TOO_SMALL;
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)2 * W * V * sizeof(float);        // the row values live in LDS where they fit, else in the workspace
#define BEAM_LM_LAUNCH(LOGITS, IN_LDS, BYTES)                                                                                  \
    do {                                                                                                                       \
        IA_SET_MAX_LDS_ONCE((ctc_prefix_beam_lm<LOGITS, IN_LDS>), BYTES);                                                      \
        hipLaunchKernelGGL((ctc_prefix_beam_lm<LOGITS, IN_LDS>), dim3(B), dim3(BEAM_THREADS), BYTES, st, x, lse, in_lens, T, ld, V, \
                           blank, W, token_min_logp, *lm, alpha, beta, tokens, lengths, scores, (unsigned char*)workspace,     \
                           w.per_utt, w.base.nodes_bytes, w.base.per_utt, w.rows_bytes, w.base.table);                         \
    } while (0)
    if (lds <= LM_LDS_ROWS_MAX) {
        if (lse) BEAM_LM_LAUNCH(true, true, lds);
        else BEAM_LM_LAUNCH(false, true, lds);
    } else {
        if (lse) BEAM_LM_LAUNCH(true, false, 0);
        else BEAM_LM_LAUNCH(false, false, 0);
    }
#undef BEAM_LM_LAUNCH
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}
