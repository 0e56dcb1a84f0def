// Transducer beam search: alignment-length synchronous decoding (Saon et al. 2020; NeMo's align_length_sync_decoding as written,
// its recombine_hypotheses included) -- the whole search of a batch in ONE launch, one workgroup per utterance, nothing waits on
// another workgroup.  The definition is in include/indicasr.h and in decoding.beam_rnnt_alsd_host.
//
// Per alignment step i the at most 16 live hypotheses are the rows of one skinny GEMM against the head; the winners that are new
// label extensions are the rows of the cell (W_hh) and W_pred GEMMs: every weight matrix is read once per step for all rows.
//   bf16 weights: mfma_f32_16x16x32_bf16.  The head's operand relu(f_t + g) is rounded to bf16 (the rounding contract of the
//     greedy MFMA decode); the unrounded fp32 h reaches the matrix cores as a three-term bf16 split h = h1 + h2 + h3 (each
//     residual is exact in fp32, 3 x 8 significant bits = fp32's 24), so the cell and W_pred products see h exactly.
//   fp32 weights: fp32 FMA, one output column per thread over all 16 rows.
// State: 2 W + 1 slots of (h, c, g) per utterance in the workspace (the last one stays zero: the parent of the start hypothesis);
// a blank winner keeps its slot, a label winner takes a slot no live member holds.  The same workgroup writes and reads them,
// ordered by barriers.  Logits, candidate keys and the beam records are in LDS.
// Identity of sequences: the canonical trie of ctc_beam.h ((parent, token) -> node through an open-addressing table); the
// emitted tokens and their alignment steps are a second, non-canonical chain of (parent, token, step) records, because two
// members with the same sequence keep their own steps.  No float atomics: two launches agree bit for bit.
#include "ctc_beam.h"

namespace {

constexpr int RB_MAX_W = 16;
constexpr int RB_THREADS = 512;
constexpr int RB_WAVES = RB_THREADS / IA_WAVE;
constexpr int RB_SLOTS = 2 * RB_MAX_W + 1;
constexpr int RB_ROWS = 16;                       // the M of the MFMA tile
constexpr int RB_CAND = RB_MAX_W + 1;             // candidates of a row: the blank and at most 16 labels
constexpr int RB_LDS_LIMIT = 160 * 1024;

typedef __bf16 rb_bf8 __attribute__((ext_vector_type(8)));
typedef float rb_f4 __attribute__((ext_vector_type(4)));

struct RbWs {
    long long recs, fcap;
    int table;
    size_t off_state, off_gates, off_rec, off_node, off_table, off_fin, per_utt, total;
};

static inline bool rb_ws_layout(int B, int T, int Hp, int Hj, int W, int max_umax, RbWs* w) {
    if (B <= 0 || T <= 0 || Hp <= 0 || Hj <= 0 || W < 1 || W > RB_MAX_W || max_umax < 0) return false;
    w->recs = 1 + (long long)W * ((long long)T + max_umax);     // the root and at most `beam` new records per step
    w->fcap = (long long)W * ((long long)max_umax + 1);
    if (w->recs > (1ll << 27) || w->fcap > (1ll << 27)) return false;
    int table = 64;
    while (table < 2 * w->recs) table <<= 1;                     // load <= 1/2: a probe always meets an empty slot
    w->table = table;
    size_t o = 0;
    w->off_state = o; o += ia_align_up((size_t)RB_SLOTS * (2 * (size_t)Hp + Hj) * sizeof(float), 256);
    w->off_gates = o; o += ia_align_up((size_t)RB_ROWS * 4 * Hp * sizeof(float), 256);
    w->off_rec = o; o += ia_align_up((size_t)w->recs * 3 * sizeof(int), 256);
    w->off_node = o; o += ia_align_up((size_t)w->recs * sizeof(int2), 256);
    w->off_table = o; o += ia_align_up((size_t)table * sizeof(int), 256);
    w->off_fin = o; o += ia_align_up((size_t)w->fcap * 3 * sizeof(int), 256);
    w->per_utt = o;
    w->total = o * (size_t)B;
    return true;
}

static inline size_t rb_lds_bytes(int Hp, int Hj, int V, bool bf16w) {
    const int K = Hp > Hj ? Hp : Hj;
    const size_t a = bf16w ? (size_t)3 * RB_ROWS * (K + 8) * 2 : (size_t)RB_ROWS * (K + 4) * 4;
    const size_t vp = (size_t)(V + 15) / 16 * 16;
    return ia_align_up(a, 16) + RB_ROWS * vp * 4 + 4096;
}

struct RbArgs {
    const float* f_all; const int64_t* lens; const int* u_max; const float* EW;
    const void* Whh; const void* Wpred; const float* bpred; const void* Whead; const float* bhead;
    int B, T, Hp, Hj, V, W, K, max_len, max_umax, score_norm;
    int *tokens, *steps, *lengths; float* scores; int* n_finished;
    char* ws; RbWs lay;
};

// The small records of the search, in LDS.
struct RbShared {
    float m_score[RB_MAX_W]; int m_u[RB_MAX_W], m_seq[RB_MAX_W], m_rec[RB_MAX_W], m_slot[RB_MAX_W];   // the beam B
    int row_m[RB_ROWS], row_t[RB_ROWS], row_slot[RB_ROWS], fidx[RB_ROWS];                             // the live rows
    float c_score[RB_ROWS * RB_CAND]; int c_tok[RB_ROWS * RB_CAND];                                   // A: per row blank, labels
    int win[RB_MAX_W];
    float n_score[RB_MAX_W]; int n_u[RB_MAX_W], n_seq[RB_MAX_W], n_rec[RB_MAX_W], n_slot[RB_MAX_W], n_fin[RB_MAX_W], n_first[RB_MAX_W];
    int new_slot[RB_ROWS], new_parent[RB_ROWS], new_tok[RB_ROWS];                                     // the rows of the cell GEMM
    unsigned long long red[RB_WAVES];
    int pick[RB_MAX_W];
    int nB, nlive, nwin, nnew, nrec, nseq, nF, npick;
};

__device__ __forceinline__ unsigned short rb_bf16_bits(float v) {
    union { __bf16 h; unsigned short u; } p;
    p.h = (__bf16)v;
    return p.u;
}
__device__ __forceinline__ float rb_bf16_value(unsigned short u) { return __uint_as_float((unsigned)u << 16); }

// out(r, o) = sum over terms and k of A_term[r][k] W[o][k]; r < 16, o < N.  A: bf16 in LDS, [terms][16][lda]; W: bf16 row-major [N][K],
// K a multiple of 32.  A wave owns tiles of 16 outputs; lane l multiplies row l & 15 of A with weight row o = 16 tile + (l & 15) over the
// k chunk 8 (l >> 4) of every 32, and ends with out[4 (l >> 4) + j][o] in acc[j].
template <int TERMS, typename Epi>
__device__ __forceinline__ void rb_gemm_mfma(const unsigned short* A, int lda, const unsigned short* W, int N, int K, Epi epi) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c16 = lane & 15, q4 = lane >> 4, nks = K / 32;
    const int ntiles = (N + 15) / 16;
    for (int tile = wave; tile < ntiles; tile += RB_WAVES) {
        const int o = tile * 16 + c16, orow = o < N ? o : N - 1;
        const unsigned short* wrow = W + (size_t)orow * K + q4 * 8;
        const unsigned short* arow = A + (size_t)c16 * lda + q4 * 8;
        rb_f4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < nks; k0 += 4) {
            rb_bf8 wf[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int ks = k0 + i < nks ? k0 + i : nks - 1;
                wf[i] = *reinterpret_cast<const rb_bf8*>(wrow + ks * 32);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (k0 + i < nks) {
#pragma unroll
                    for (int t = TERMS - 1; t >= 0; --t) {     // the smallest term first
                        const rb_bf8 af = *reinterpret_cast<const rb_bf8*>(arow + (size_t)t * RB_ROWS * lda + (k0 + i) * 32);
                        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, wf[i], acc, 0, 0, 0);
                    }
                }
        }
        if (o < N) {
#pragma unroll
            for (int j = 0; j < 4; ++j) epi(4 * q4 + j, o, acc[j]);
        }
    }
}

// The same product in fp32: A fp32 in LDS [16][lda], W fp32 row-major [N][K], K a multiple of 4; a thread owns an output column.
template <typename Epi>
__device__ __forceinline__ void rb_gemm_f32(const float* A, int lda, const float* W, int N, int K, Epi epi) {
    const int k4n = K / 4;
    for (int o = threadIdx.x; o < N; o += RB_THREADS) {
        float acc[RB_ROWS];
#pragma unroll
        for (int r = 0; r < RB_ROWS; ++r) acc[r] = 0.f;
        const float4* w = reinterpret_cast<const float4*>(W + (size_t)o * K);
        for (int k4 = 0; k4 < k4n; ++k4) {
            const float4 wv = w[k4];
#pragma unroll
            for (int r = 0; r < RB_ROWS; ++r) {
                const float4 av = *reinterpret_cast<const float4*>(A + (size_t)r * lda + 4 * k4);
                acc[r] = fmaf(av.x, wv.x, acc[r]); acc[r] = fmaf(av.y, wv.y, acc[r]);
                acc[r] = fmaf(av.z, wv.z, acc[r]); acc[r] = fmaf(av.w, wv.w, acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < RB_ROWS; ++r) epi(r, o, acc[r]);
    }
}

template <bool BF16, typename Epi>
__device__ __forceinline__ void rb_gemm(const void* A, int lda, int terms, const void* W, int N, int K, Epi epi) {
    if constexpr (BF16) {
        if (terms == 1) rb_gemm_mfma<1>((const unsigned short*)A, lda, (const unsigned short*)W, N, K, epi);
        else rb_gemm_mfma<3>((const unsigned short*)A, lda, (const unsigned short*)W, N, K, epi);
    } else {
        rb_gemm_f32((const float*)A, lda, (const float*)W, N, K, epi);
    }
}

// One fp32 value into the operand of the next GEMM: unrounded (fp32 weights), rounded to bf16 (`terms` 1: the head), or as the
// exact three-term bf16 split.
template <bool BF16>
__device__ __forceinline__ void rb_put(void* A, int lda, int terms, int r, int k, float v) {
    if constexpr (BF16) {
        unsigned short* a = (unsigned short*)A;
        const unsigned short b1 = rb_bf16_bits(v);
        a[(size_t)r * lda + k] = b1;
        if (terms == 3) {
            const float r1 = v - rb_bf16_value(b1);
            const unsigned short b2 = rb_bf16_bits(r1);
            const float r2 = r1 - rb_bf16_value(b2);
            a[(size_t)(RB_ROWS + r) * lda + k] = b2;
            a[(size_t)(2 * RB_ROWS + r) * lda + k] = rb_bf16_bits(r2);
        }
    } else {
        ((float*)A)[(size_t)r * lda + k] = v;
    }
}

__device__ __forceinline__ float rb_logaddexp(float a, float b) {
    const float mx = fmaxf(a, b), mn = fminf(a, b);
    if (mn == IA_NEG_INF) return mx;
    return mx + log1pf(expf(mn - mx));
}
__device__ __forceinline__ float rb_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ int rb_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The largest key of the workgroup (0: none); every thread gets it.
__device__ __forceinline__ unsigned long long rb_block_max(unsigned long long v, unsigned long long* red) {
    const unsigned long long w = beam_wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
    __syncthreads();
    unsigned long long m = red[0];
#pragma unroll
    for (int i = 1; i < RB_WAVES; ++i) m = red[i] > m ? red[i] : m;
    return m;
}

template <bool BF16>
__global__ __launch_bounds__(RB_THREADS, 1) void rnnt_beam_alsd_kernel(RbArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rb_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const int Hp = a.Hp, Hj = a.Hj, V = a.V, T = a.T, blank = V - 1;
    const int beam = a.W < V - 1 ? a.W : V - 1;
    const int Kmax = Hp > Hj ? Hp : Hj;
    const int lda = BF16 ? Kmax + 8 : Kmax + 4;
    const int Vp = (V + 15) / 16 * 16;
    const size_t a_bytes = ((BF16 ? (size_t)3 * RB_ROWS * lda * 2 : (size_t)RB_ROWS * lda * 4) + 15) / 16 * 16;
    void* Aop = rb_smem;
    float* logits = reinterpret_cast<float*>(rb_smem + a_bytes);
    RbShared& S = *reinterpret_cast<RbShared*>(rb_smem + a_bytes + (size_t)RB_ROWS * Vp * 4);

    char* ws = a.ws + (size_t)b * a.lay.per_utt;
    float* state = reinterpret_cast<float*>(ws + a.lay.off_state);
    float* gates = reinterpret_cast<float*>(ws + a.lay.off_gates);
    int* rec = reinterpret_cast<int*>(ws + a.lay.off_rec);            // [recs][3]: parent, token, step
    int2* node = reinterpret_cast<int2*>(ws + a.lay.off_node);
    int* table = reinterpret_cast<int*>(ws + a.lay.off_table);
    int* fin = reinterpret_cast<int*>(ws + a.lay.off_fin);            // [fcap][3]: record, score bits, u
    const int nrec_cap = (int)a.lay.recs, fcap = (int)a.lay.fcap, tmask = a.lay.table - 1;
    const size_t slot_stride = 2 * (size_t)Hp + Hj;
    auto slot_h = [&](int s) { return state + (size_t)s * slot_stride; };
    auto slot_c = [&](int s) { return state + (size_t)s * slot_stride + Hp; };
    auto slot_g = [&](int s) { return state + (size_t)s * slot_stride + 2 * Hp; };

    long long len64 = a.lens[b];
    const int len = (int)(len64 < 0 ? 0 : (len64 > T ? T : len64));
    const int u_max = rb_clamp(a.u_max[b], 0, a.max_umax);
    const int nsteps = len + u_max;

    // ---- start: the table empty, the zero slot, B = [((blank), 0, [])]
    for (int i = tid; i < a.lay.table; i += RB_THREADS) table[i] = -1;
    for (int i = tid; i < (int)slot_stride; i += RB_THREADS) slot_h(RB_SLOTS - 1)[i] = 0.f;
    if (tid == 0) {
        S.nB = 1; S.nrec = 1; S.nseq = 1; S.nF = 0; S.npick = 0;
        S.m_score[0] = 0.f; S.m_u[0] = 0; S.m_seq[0] = 0; S.m_rec[0] = 0; S.m_slot[0] = 0;
        rec[0] = 0; rec[1] = -1; rec[2] = -1;
        node[0] = make_int2(-1, -1);
        S.nnew = nsteps > 0 ? 1 : 0;                       // the state of (blank): the cell on EW[blank] from the zero state
        S.new_slot[0] = 0; S.new_parent[0] = RB_SLOTS - 1; S.new_tok[0] = blank;
    }
    __syncthreads();

    for (int i = -1; i < nsteps; ++i) {
        if (i >= 0) {
            // ---- the live members, in B's order
            if (tid == 0) {
                int n = 0;
                for (int m = 0; m < S.nB; ++m) {
                    const int t = i - S.m_u[m];
                    if (t <= len - 1 && n < RB_ROWS) {
                        S.row_m[n] = m; S.row_t[n] = rb_clamp(t, 0, T - 1); S.row_slot[n] = rb_clamp(S.m_slot[m], 0, RB_SLOTS - 1);
                        ++n;
                    }
                }
                S.nlive = n;
            }
            __syncthreads();
            const int nlive = S.nlive;
            if (nlive == 0) break;
            // ---- head: logits[r] = W_head act(f[t_r] + g_r) + b_head
            for (int idx = tid; idx < RB_ROWS * Hj; idx += RB_THREADS) {
                const int r = idx / Hj, k = idx - r * Hj;
                float v = 0.f;
                if (r < nlive) v = fmaxf(a.f_all[((size_t)b * T + S.row_t[r]) * Hj + k] + slot_g(S.row_slot[r])[k], 0.f);
                rb_put<BF16>(Aop, lda, 1, r, k, v);
            }
            __syncthreads();
            rb_gemm<BF16>(Aop, lda, 1, a.Whead, V, Hj, [&](int r, int o, float x) { logits[(size_t)r * Vp + o] = x + a.bhead[o]; });
            __syncthreads();
            // ---- per row: log-softmax, the blank candidate, the `beam` largest labels (equal values: the smaller id)
            for (int r = wave; r < nlive; r += RB_WAVES) {
                const float* L = logits + (size_t)r * Vp;
                float mx = -INFINITY;
                for (int v = lane; v < V; v += 64) mx = fmaxf(mx, L[v]);
                mx = ia_wave_max(mx);
                float sum = 0.f;
                for (int v = lane; v < V; v += 64) sum += expf(L[v] - mx);
                sum = ia_wave_sum(sum);
                const float lse = mx + logf(sum);
                const float base = S.m_score[S.row_m[r]];
                if (lane == 0) { S.c_score[r * RB_CAND] = base + (L[blank] - lse); S.c_tok[r * RB_CAND] = blank; }
                unsigned long long last = ~0ull;
                for (int j = 0; j < beam; ++j) {
                    unsigned long long best = 0;
                    for (int v = lane; v < blank; v += 64) {
                        const unsigned long long key = beam_key(L[v], v);
                        if (key < last && key > best) best = key;
                    }
                    best = beam_wave_max(best);
                    last = best;
                    if (lane == 0) {
                        const int id = rb_clamp((int)(0xffffffffu - (uint32_t)(best & 0xffffffffu)), 0, blank > 0 ? blank - 1 : 0);
                        S.c_score[r * RB_CAND + 1 + j] = base + (L[id] - lse);
                        S.c_tok[r * RB_CAND + 1 + j] = id;
                    }
                }
            }
            __syncthreads();
            // ---- the first `beam` of A by descending score, stable: key = (orderable score, complemented position in A)
            if (wave == 0) {
                const int per = beam + 1, ncand = nlive * per;
                unsigned long long last = ~0ull;
                const int nwin = ncand < beam ? ncand : beam;
                for (int w = 0; w < nwin; ++w) {
                    unsigned long long best = 0;
                    for (int p = lane; p < ncand; p += 64) {
                        const int r = p / per, j = p - r * per;
                        const unsigned long long key = beam_key(S.c_score[r * RB_CAND + j], p);
                        if (key < last && key > best) best = key;
                    }
                    best = beam_wave_max(best);
                    last = best;
                    if (lane == 0) S.win[w] = rb_clamp((int)(0xffffffffu - (uint32_t)(best & 0xffffffffu)), 0, ncand - 1);
                }
                if (lane == 0) S.nwin = nwin;
            }
            __syncthreads();
            // ---- the records: finished list, the new B, sequence identity, recombination, slots
            if (tid == 0) {
                const int per = beam + 1;
                unsigned long long oldmask = 0;
                for (int r = 0; r < nlive; ++r) {
                    const int m = S.row_m[r];
                    oldmask |= 1ull << S.row_slot[r];
                    S.fidx[r] = -1;
                    if (i - S.m_u[m] == len - 1 && S.nF < fcap) {      // its blank candidate is final, pruned or not
                        const int f = S.nF++;
                        fin[3 * f] = S.m_rec[m]; fin[3 * f + 1] = __float_as_int(S.c_score[r * RB_CAND]); fin[3 * f + 2] = S.m_u[m];
                        S.fidx[r] = f;
                    }
                }
                int nnew = 0, next_free = 0;
                for (int w = 0; w < S.nwin; ++w) {
                    const int p = S.win[w], r = p / per, j = p - r * per, m = S.row_m[r];
                    S.n_score[w] = S.c_score[r * RB_CAND + j];
                    if (j == 0) {
                        S.n_u[w] = S.m_u[m]; S.n_seq[w] = S.m_seq[m]; S.n_rec[w] = S.m_rec[m]; S.n_slot[w] = S.row_slot[r];
                        S.n_fin[w] = S.fidx[r];
                    } else {
                        const int tok = S.c_tok[r * RB_CAND + j], parent = S.m_seq[m];
                        int id = -1;
                        unsigned h = beam_hash(parent, tok) & tmask;
                        for (int probe = 0; probe <= tmask; ++probe) {       // bounded by the table
                            const int e = table[h];
                            if (e < 0) {
                                if (S.nseq < nrec_cap) { id = S.nseq++; node[id] = make_int2(parent, tok); table[h] = id; }
                                break;
                            }
                            const int2 nd = node[rb_clamp(e, 0, nrec_cap - 1)];
                            if (nd.x == parent && nd.y == tok) { id = e; break; }
                            h = (h + 1) & tmask;
                        }
                        int rc = S.nrec < nrec_cap ? S.nrec++ : nrec_cap - 1;
                        rec[3 * rc] = S.m_rec[m]; rec[3 * rc + 1] = tok; rec[3 * rc + 2] = i;
                        while (next_free < RB_SLOTS - 1 && ((oldmask >> next_free) & 1ull)) ++next_free;
                        const int slot = next_free < RB_SLOTS - 1 ? next_free++ : RB_SLOTS - 2;
                        S.n_u[w] = S.m_u[m] + 1; S.n_seq[w] = id; S.n_rec[w] = rc; S.n_slot[w] = slot; S.n_fin[w] = -1;
                        S.new_slot[nnew] = slot; S.new_parent[nnew] = S.row_slot[r]; S.new_tok[nnew] = tok;
                        ++nnew;
                    }
                }
                // recombine_hypotheses as written: a later member of an earlier sequence adds its score to the first occurrence
                // and stays in B with its own
                for (int w = 0; w < S.nwin; ++w) {
                    int first = -1;
                    for (int q = 0; q < w; ++q)
                        if (S.n_first[q] && S.n_seq[q] == S.n_seq[w]) { first = q; break; }
                    S.n_first[w] = first < 0;
                    if (first >= 0) S.n_score[first] = rb_logaddexp(S.n_score[first], S.n_score[w]);
                }
                for (int w = 0; w < S.nwin; ++w) {
                    if (S.n_fin[w] >= 0) fin[3 * S.n_fin[w] + 1] = __float_as_int(S.n_score[w]);     // the same record
                    S.m_score[w] = S.n_score[w]; S.m_u[w] = S.n_u[w]; S.m_seq[w] = S.n_seq[w]; S.m_rec[w] = S.n_rec[w];
                    S.m_slot[w] = S.n_slot[w];
                }
                S.nB = S.nwin;
                S.nnew = nnew;
            }
            __syncthreads();
        }
        const int nnew = S.nnew;
        if (nnew == 0 || i == nsteps - 1) continue;        // no new sequence survived (or nothing is evaluated after this step)
        // ---- the cell of the new sequences: gates = W_hh h_parent + EW[token]
        for (int idx = tid; idx < RB_ROWS * Hp; idx += RB_THREADS) {
            const int r = idx / Hp, k = idx - r * Hp;
            rb_put<BF16>(Aop, lda, 3, r, k, r < nnew ? slot_h(S.new_parent[r])[k] : 0.f);
        }
        __syncthreads();
        rb_gemm<BF16>(Aop, lda, 3, a.Whh, 4 * Hp, Hp, [&](int r, int o, float x) { if (r < nnew) gates[(size_t)r * 4 * Hp + o] = x; });
        __syncthreads();
        for (int idx = tid; idx < RB_ROWS * Hp; idx += RB_THREADS) {
            const int r = idx / Hp, k = idx - r * Hp;
            float hn = 0.f;
            if (r < nnew) {
                const float* e = a.EW + (size_t)rb_clamp(S.new_tok[r], 0, V) * 4 * Hp;
                const float* g = gates + (size_t)r * 4 * Hp;
                const float gi = rb_sigmoid(g[k] + e[k]), gf = rb_sigmoid(g[Hp + k] + e[Hp + k]);
                const float gg = tanhf(g[2 * Hp + k] + e[2 * Hp + k]), go = rb_sigmoid(g[3 * Hp + k] + e[3 * Hp + k]);
                const float cn = gf * slot_c(S.new_parent[r])[k] + gi * gg;
                hn = go * tanhf(cn);
                slot_c(S.new_slot[r])[k] = cn;
                slot_h(S.new_slot[r])[k] = hn;
            }
            rb_put<BF16>(Aop, lda, 3, r, k, hn);           // the operand of W_pred (the gates GEMM is behind a barrier)
        }
        __syncthreads();
        rb_gemm<BF16>(Aop, lda, 3, a.Wpred, Hj, Hp, [&](int r, int o, float x) { if (r < nnew) slot_g(S.new_slot[r])[o] = x + a.bpred[o]; });
        __syncthreads();
    }
    __syncthreads();

    // ---- the result: F by descending score / (u + 1) (or score), stable; B as it stands when F is empty
    const int K = a.K, nF = S.nF;
    int npick = 0;
    if (nF > 0) {
        unsigned long long last = ~0ull;
        npick = nF < K ? nF : K;
        for (int r = 0; r < npick; ++r) {
            unsigned long long best = 0;
            for (int f = tid; f < nF; f += RB_THREADS) {
                const float sc = __int_as_float(fin[3 * f + 1]);
                const float key_score = a.score_norm ? sc / (float)(fin[3 * f + 2] + 1) : sc;
                const unsigned long long key = beam_key(key_score, f);
                if (key < last && key > best) best = key;
            }
            best = rb_block_max(best, S.red);
            last = best;
            if (tid == 0) S.pick[r] = rb_clamp((int)(0xffffffffu - (uint32_t)(best & 0xffffffffu)), 0, nF - 1);
        }
    } else {
        npick = S.nB < K ? S.nB : K;
    }
    __syncthreads();
    int* tokens = a.tokens + (size_t)b * K * a.max_len;
    int* steps = a.steps + (size_t)b * K * a.max_len;
    for (int idx = tid; idx < K * a.max_len; idx += RB_THREADS) { tokens[idx] = -1; steps[idx] = -1; }
    __syncthreads();
    if (tid < K) {
        int u = -1, rc = 0;
        float sc = -INFINITY;
        if (tid < npick) {
            if (nF > 0) { const int f = S.pick[tid]; rc = fin[3 * f]; sc = __int_as_float(fin[3 * f + 1]); u = fin[3 * f + 2]; }
            else { rc = S.m_rec[tid]; sc = S.m_score[tid]; u = S.m_u[tid]; }
            u = rb_clamp(u, 0, a.max_len);
            for (int s = u - 1; s >= 0; --s) {
                rc = rb_clamp(rc, 0, nrec_cap - 1);
                tokens[(size_t)tid * a.max_len + s] = rec[3 * rc + 1];
                steps[(size_t)tid * a.max_len + s] = rec[3 * rc + 2];
                rc = rec[3 * rc];
            }
        }
        a.lengths[(size_t)b * K + tid] = u;
        a.scores[(size_t)b * K + tid] = sc;
    }
    if (tid == 0) a.n_finished[b] = nF;
}

int rb_launch(const float* f_all, const int64_t* lens, const int* u_max, const float* EW, const void* Whh, const void* Wpred,
              const float* bpred, const void* Whead, const float* bhead, int B, int T, int Hp, int Hj, int V, int W, int K,
              int max_umax, int score_norm, int* tokens, int* steps, int* lengths, float* scores, int* n_finished, void* ws,
              size_t ws_bytes, bool bf16w, ia_stream_t stream) {
    if (!f_all || !lens || !u_max || !EW || !Whh || !Wpred || !bpred || !Whead || !bhead || !tokens || !steps || !lengths || !scores ||
        !n_finished || !ws || B <= 0 || T <= 0 || Hp <= 0 || Hj <= 0 || V < 2 || W < 1 || K < 1 || max_umax < 0)
        return IA_INVALID_VALUE;
    if (!ia_is_aligned(f_all, 16) || !ia_is_aligned(EW, 16) || !ia_is_aligned(Whh, 16) || !ia_is_aligned(Wpred, 16) ||
        !ia_is_aligned(Whead, 16) || !ia_is_aligned(lens, 8) || !ia_is_aligned(u_max, 4) || !ia_is_aligned(bpred, 4) ||
        !ia_is_aligned(bhead, 4) || !ia_is_aligned(tokens, 4) || !ia_is_aligned(steps, 4) || !ia_is_aligned(lengths, 4) ||
        !ia_is_aligned(scores, 4) || !ia_is_aligned(n_finished, 4) || !ia_is_aligned(ws, 256))
        return IA_INVALID_VALUE;
    if (W > RB_MAX_W || K > RB_MAX_W) return IA_UNSUPPORTED;
    if (bf16w ? (Hp % 32 != 0 || Hj % 32 != 0) : (Hp % 4 != 0 || Hj % 4 != 0)) return IA_UNSUPPORTED;
    const size_t lds = rb_lds_bytes(Hp, Hj, V, bf16w);
    if (lds > (size_t)RB_LDS_LIMIT || sizeof(RbShared) > 4096) return IA_UNSUPPORTED;
    RbArgs a;
    if (!rb_ws_layout(B, T, Hp, Hj, W, max_umax, &a.lay)) return IA_UNSUPPORTED;
    if (ws_bytes < a.lay.total) return IA_WORKSPACE_TOO_SMALL;
    a.f_all = f_all; a.lens = lens; a.u_max = u_max; a.EW = EW; a.Whh = Whh; a.Wpred = Wpred; a.bpred = bpred; a.Whead = Whead;
    a.bhead = bhead; a.B = B; a.T = T; a.Hp = Hp; a.Hj = Hj; a.V = V; a.W = W; a.K = K; a.max_len = T + max_umax; a.max_umax = max_umax;
    a.score_norm = score_norm; a.tokens = tokens; a.steps = steps; a.lengths = lengths; a.scores = scores; a.n_finished = n_finished;
    a.ws = (char*)ws;
    if (bf16w) {
        IA_SET_MAX_LDS_ONCE(rnnt_beam_alsd_kernel<true>, (int)lds);
        hipLaunchKernelGGL(rnnt_beam_alsd_kernel<true>, dim3(B), dim3(RB_THREADS), lds, (hipStream_t)stream, a);
    } else {
        IA_SET_MAX_LDS_ONCE(rnnt_beam_alsd_kernel<false>, (int)lds);
        hipLaunchKernelGGL(rnnt_beam_alsd_kernel<false>, dim3(B), dim3(RB_THREADS), lds, (hipStream_t)stream, a);
    }
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}

}  // namespace

extern "C" int ia_rnnt_beam_max_width(void) { return RB_MAX_W; }

extern "C" size_t ia_rnnt_beam_workspace_bytes(int B, int T, int Hp, int Hj, int V, int W, int max_umax) {
    RbWs w;
    if (V < 2 || !rb_ws_layout(B, T, Hp, Hj, W, max_umax, &w)) return 0;
    return w.total;
}

extern "C" int ia_rnnt_beam_alsd(const float* f_all, const int64_t* lens, const int32_t* u_max, const float* EW, const float* Whh,
                                 const float* Wpred, const float* bpred, const float* Whead, const float* bhead, int B, int T, int Hp,
                                 int Hj, int V, int W, int K, int max_umax, int score_norm, int32_t* tokens, int32_t* steps,
                                 int32_t* lengths, float* scores, int32_t* n_finished, void* workspace, size_t workspace_bytes,
                                 ia_stream_t stream) {
    return rb_launch(f_all, lens, u_max, EW, Whh, Wpred, bpred, Whead, bhead, B, T, Hp, Hj, V, W, K, max_umax, score_norm, tokens, steps,
                     lengths, scores, n_finished, workspace, workspace_bytes, false, stream);
}

extern "C" int ia_rnnt_beam_alsd_bf16w(const float* f_all, const int64_t* lens, const int32_t* u_max, const float* EW,
                                       const void* Whh_bf16, const void* Wpred_bf16, const float* bpred, const void* Whead_bf16,
                                       const float* bhead, int B, int T, int Hp, int Hj, int V, int W, int K, int max_umax,
                                       int score_norm, int32_t* tokens, int32_t* steps, int32_t* lengths, float* scores,
                                       int32_t* n_finished, void* workspace, size_t workspace_bytes, ia_stream_t stream) {
    return rb_launch(f_all, lens, u_max, EW, Whh_bf16, Wpred_bf16, bpred, Whead_bf16, bhead, B, T, Hp, Hj, V, W, K, max_umax, score_norm,
                     tokens, steps, lengths, scores, n_finished, workspace, workspace_bytes, true, stream);
}
