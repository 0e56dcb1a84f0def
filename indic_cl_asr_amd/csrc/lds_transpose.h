// Row-major LDS tiles of 16-bit elements read back COLUMN-wise with gfx950's transposing LDS read (gemm_tn.hip, joint_dw.hip).
// Both operands of a weight-gradient GEMM are row-major over the contracted index, so an MFMA fragment (8 consecutive contracted
// rows of one output row / column) is a column of the tile as it lies in memory.  ds_read_b64_tr_b16 fetches, per 16-lane group, a
// 4-row x 16-column block and hands lane i column i; two of them form one 16x16x32 operand fragment.
// rowb = LDS bytes per tile row (a multiple of 256); WIDE = the chunk index may exceed 15 (the general form, valid for 16-chunk rows
// too: joint_dw.hip uses it for both its tiles, gemm_tn.hip the short one); V4 = the 4-element vector type of the tile's elements.
// rowb is a function argument, not a template parameter, on purpose: with the pitch folded in before inlining, the weight-gradient
// kernel of the joint, which sits at the edge of the register file, spills more (profiles/joint_dw_refactor.md).
#pragma once

namespace {

// byte offset of 16-byte chunk ch of row `row`: the low 4 bits of the chunk index are XOR-swizzled (cdna_hip_programming.md T10,
// image b) so that the row-wise stores and the transposed 4-row block reads are both conflict-free
template <bool WIDE>
__device__ __forceinline__ int trl_off(int rowb, int row, int ch) {
    if constexpr (WIDE) return rowb * row + 16 * ((ch & ~15) | ((ch & 15) ^ (((row & 3) << 2) | ((row >> 2) & 3))));
    else return rowb * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}

// LDS byte addresses (address space 3) of the two 4-row blocks of one 16x16x32 operand fragment: 8 consecutive contracted rows
// r0 .. r0+7 for column col0 + (lane & 15).  Lane 4q+p of a 16-lane group addresses row q, columns 4p .. 4p+3 of its block.
template <bool WIDE>
__device__ __forceinline__ void trl_frag_addr(unsigned tile_lds, int rowb, int r0, int col0, int lane, unsigned* a0, unsigned* a1) {
    const int l16 = lane & 15, q = l16 >> 2, p = l16 & 3;
    const int ch = (col0 >> 3) + (p >> 1);
    *a0 = tile_lds + trl_off<WIDE>(rowb, r0 + q, ch) + 8 * (p & 1);
    *a1 = tile_lds + trl_off<WIDE>(rowb, r0 + 4 + q, ch) + 8 * (p & 1);
}

// one transposed block at addr + OFF bytes (an immediate: rows further down the tile in the same swizzle phase).  The read is
// asynchronous and the compiler does not know it: the caller ties the results to ONE s_waitcnt lgkmcnt(0) before it uses them.
template <class V4, int OFF = 0>
__device__ __forceinline__ V4 trl_read(unsigned addr) {
    V4 v;
    if constexpr (OFF == 0) asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v) : "v"(addr));
    else asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
    return v;
}

// the fragment (8 elements) of its two blocks
template <class V4>
__device__ __forceinline__ auto trl_join(V4 lo, V4 hi) {
    decltype(__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7)) o;
#pragma unroll
    for (int j = 0; j < 4; ++j) { o[j] = lo[j]; o[4 + j] = hi[j]; }
    return o;
}
}  // namespace
