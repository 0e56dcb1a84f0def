// What the two CTC prefix beam search kernels share (csrc/ctc_beam.hip, csrc/ctc_beam_lm.hip): the limits, the workspace of the
// prefix trie, the 64-bit ordered candidate keys and their wave maximum, the trie's hash and loads.
#pragma once
#include "ia_common.h"

namespace {

constexpr int BEAM_MAX_W = 32;
constexpr int BEAM_MAX_V = 1024;
constexpr int BEAM_THREADS = 256;
constexpr int BEAM_WAVES = BEAM_THREADS / IA_WAVE;
constexpr int BEAM_TOK = BEAM_MAX_V / BEAM_THREADS;   // tokens a thread owns at most
constexpr int BEAM_PF = 4;                            // frames in the LDS ring

struct BeamWs { int table; size_t nodes_bytes, per_utt, total; };

static inline bool beam_ws_layout(int B, int T, int V, int W, BeamWs* w) {
    if (W < 1 || W > BEAM_MAX_W || V > BEAM_MAX_V) return false;
    const long long nodes = 1 + (long long)W * T;     // the root and at most W new prefixes per frame
    if (nodes > (1ll << 28)) return false;
    int table = 64;
    while (table < 2 * nodes) table <<= 1;            // load <= 1/2: a probe always meets an empty slot
    w->table = table;
    w->nodes_bytes = ia_align_up((size_t)nodes * sizeof(int2), 256);
    w->per_utt = w->nodes_bytes + ia_align_up((size_t)table * sizeof(int), 256);
    w->total = w->per_utt * (size_t)B;
    return true;
}

__device__ __forceinline__ uint32_t beam_ord(float f) {          // monotone float -> uint
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float beam_unord(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
// larger score first, then the smaller id; never 0 for a number
__device__ __forceinline__ unsigned long long beam_key(float score, int id) {
    return ((unsigned long long)beam_ord(score + 0.f) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)id);
}
// 64-lane unsigned maximum on DPP alone (the steps of ia_wave_max_dpp), wave-uniform result
__device__ __forceinline__ uint32_t beam_dpp_umax_step(uint32_t v, uint32_t moved) { return moved > v ? moved : v; }
#define BEAM_DPP_U(v, ctrl, rmask) ((uint32_t)__builtin_amdgcn_update_dpp((int)(v), (int)(v), ctrl, rmask, 0xF, false))
__device__ __forceinline__ uint32_t beam_wave_umax(uint32_t v) {
    v = beam_dpp_umax_step(v, BEAM_DPP_U(v, 0xB1, 0xF));
    v = beam_dpp_umax_step(v, BEAM_DPP_U(v, 0x4E, 0xF));
    v = beam_dpp_umax_step(v, BEAM_DPP_U(v, 0x141, 0xF));
    v = beam_dpp_umax_step(v, BEAM_DPP_U(v, 0x140, 0xF));
    v = beam_dpp_umax_step(v, BEAM_DPP_U(v, 0x142, 0xA));
    v = beam_dpp_umax_step(v, BEAM_DPP_U(v, 0x143, 0xC));
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
// the largest key of the wave: the largest score word, then the largest id word among the lanes that hold it (the id word of a
// candidate is never 0, and the key 0 means "none")
__device__ __forceinline__ unsigned long long beam_wave_max(unsigned long long v) {
    const uint32_t hi = beam_wave_umax((uint32_t)(v >> 32));
    const uint32_t lo = beam_wave_umax((uint32_t)(v >> 32) == hi ? (uint32_t)(v & 0xffffffffu) : 0u);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned beam_hash(int parent, int token) {
    unsigned h = (unsigned)parent * 0x9E3779B1u + (unsigned)token * 0x85EBCA77u;
    h ^= h >> 15;
    h *= 0x2C1B3C6Du;
    h ^= h >> 13;
    return h;
}
__device__ __forceinline__ int beam_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int2 beam_load_node(const int2* p) {      // (parent, token) in one 8-byte load
    const unsigned long long v = __hip_atomic_load((const unsigned long long*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return make_int2((int)(uint32_t)(v & 0xffffffffu), (int)(uint32_t)(v >> 32));
}

}  // namespace
