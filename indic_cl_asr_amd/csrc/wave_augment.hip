// Waveform augmentation in one pass over the padded batch (gfx950): speed (band-limited resampling), gain, shift and white noise
// of NeMo's train_ds.augmentor (A/parts/preprocessing/perturb.py) folded into one launch between the batch's arrival and
// ia_feat_preemph; the definition is in include/indicasr.h.
//   grid   one workgroup (256 threads) per WA_TILE = 1024 consecutive output samples of one utterance; lane = output sample, so
//          a wave reads 64 neighbouring input samples per tap (consecutive LDS banks, duplicates broadcast).
//   LDS    the input span the tile reaches: tile * sr / new_sr samples plus 2 (Z / s + 1) + 2, zero outside the utterance so that
//          the tap loops carry no bounds test, shift_pre and input-stage noise applied while staging.
//   table  read through the cache for both tables (kaiser_fast 32 KB, kaiser_best 128 KB; same code, templated on Z).  Staging the
//          kaiser_fast table in LDS behind the span was measured and dropped: 32 KB copied per 4 KB of output and half the
//          resident workgroups made the launch twice as slow.
//   taps   one 64-bit division per thread and tile gives kc = floor(j sr / new_sr) and the remainder of its first sample; the
//          next sample of the thread is 256 further, an increment with one carry.  From there (i, e q) of the definition step by
//          (new_sr P / q, new_sr P mod q) per tap with one carry, in 32-bit integers: the left wing from kc downwards and the
//          right wing from kc + 1 upwards side by side, each into its own fp32 sum, a fixed ceil(Z q / new_sr) taps per wing
//          (a tap with i >= Z P weighs 0), so the loop unrolls and its reads overlap.
//   gather across the lanes of a tap the table index i moves by sr P / q per output sample (465 entries at new_sr = 17,600, 512
//          at 14,400, where m sr mod new_sr has period 9 and a wave reads 9 distinct entries); along a lane's own taps it moves by
//          s P, 512 entries when s = 1 -- one LDS bank, one cache line per tap -- which is why taps are walked in time and never
//          spread over lanes.
// Unresampled utterances (new_sr = 0) take the copy path of the same kernel: no LDS, no table.
#include "ia_common.h"

namespace {

constexpr int WA_P = 512;            // table entries per zero crossing
constexpr int WA_TILE = 1024;        // output samples per workgroup
constexpr int WA_THREADS = 256;
constexpr int WA_MAX_SR = 1 << 20;       // 256 sr fits an int
constexpr int WA_MAX_NEW_SR = 1 << 21;   // new_sr P fits an int
constexpr int WA_LDS_BYTES = 160 * 1024;

__device__ __forceinline__ unsigned wa_hash32(unsigned x) {
    x ^= x >> 16; x *= 0x85ebca6bu; x ^= x >> 13; x *= 0xc2b2ae35u; x ^= x >> 16;
    return x;
}
// the counter-based normal of csrc/frontend.hip (fe_randn) and csrc/frontend_fft.hip (ff_randn)
__device__ __forceinline__ float wa_randn(unsigned seed, unsigned b, unsigned n) {
    const unsigned h1 = wa_hash32((b * 0x9E3779B1u) ^ (n * 0x85EBCA77u) ^ seed);
    const unsigned h2 = wa_hash32(h1 ^ 0x68E31DA4u);
    const float u1 = ((float)(h1 >> 8) + 1.0f) * (1.0f / 16777217.0f);
    const float u2 = (float)(h2 >> 8) * (1.0f / 16777216.0f);
    return sqrtf(-2.0f * __logf(u1)) * __cosf(6.28318530717958647f * u2);
}

// amp N(i) for 0 <= i < n, 0 outside
__device__ __forceinline__ float wa_noise(const ia_wave_params& p, unsigned b, int64_t i, int n) {
    return (i >= 0 && i < n) ? p.noise_amp * wa_randn(p.noise_seed, b, (unsigned)i) : 0.f;
}

// in(k) of the definition
__device__ __forceinline__ float wa_input(const ia_wave_params& p, const float* __restrict__ xr, unsigned b, int64_t k) {
    if (k < 0 || k >= p.n_in) return 0.f;
    const int64_t src = k + p.shift_pre;
    float v = (src >= 0 && src < p.n_in) ? xr[src] : 0.f;
    if (p.noise_stage == 1 && p.noise_amp != 0.f) v += wa_noise(p, b, k + p.noise_shift, p.n_in);
    return v;
}

template <int Z>
__global__ __launch_bounds__(WA_THREADS) void wave_augment_kernel(const float* __restrict__ x, int L_in, float* __restrict__ y,
                                                                  int L_out, const ia_wave_params* __restrict__ params,
                                                                  const float* __restrict__ table, int sr, int span_cap,
                                                                  int tiles_per_row) {
    extern __shared__ __attribute__((aligned(16))) float wa_lds[];
    constexpr int ZP = Z * WA_P;
    const int tid = threadIdx.x;
    const unsigned b = blockIdx.x / tiles_per_row;
    const int m0 = (int)(blockIdx.x - b * tiles_per_row) * WA_TILE;
    const int m1 = min(m0 + WA_TILE, L_out);
    ia_wave_params p = params[b];
    p.n_in = max(0, min(p.n_in, L_in));
    p.n_out = max(0, min(p.n_out, L_out));
    const float* xr = x + (size_t)b * L_in;
    float* yo = y + (size_t)b * L_out;

    if (m0 >= p.n_out) {                                   // a tile of padding
        for (int m = m0 + tid; m < m1; m += WA_THREADS) yo[m] = 0.f;
        return;
    }
    const bool out_noise = p.noise_stage == 0 && p.noise_amp != 0.f;
    if (p.new_sr == 0) {                                   // the copy path: shift, gain, noise, zero fill
        for (int m = m0 + tid; m < m1; m += WA_THREADS) {
            float v = 0.f;
            if (m < p.n_out) {
                const int64_t j = (int64_t)m + p.shift_post;
                const float r = (j >= 0 && j < p.n_out) ? wa_input(p, xr, b, j) : 0.f;
                v = p.gain * r;
                if (out_noise) v += wa_noise(p, b, (int64_t)m + p.noise_shift, p.n_out);
            }
            yo[m] = v;
        }
        return;
    }

    const int new_sr = p.new_sr;
    const int q = max(sr, new_sr);
    const int W = (int)(((int64_t)Z * q + new_sr - 1) / new_sr) + 1;       // taps per wing, one to spare
    // the resampled positions this tile reads: j = m + shift_post inside [0, n_out)
    const int64_t j_lo = max((int64_t)m0 + p.shift_post, (int64_t)0);
    const int64_t j_hi = min((int64_t)min(m1, p.n_out) - 1 + p.shift_post, (int64_t)p.n_out - 1);
    const bool any = j_lo <= j_hi;
    int64_t k_lo = 0;
    int len = 0;
    // the span of a full tile at this rate (wa_span_cap): the same verdict for every tile of the row
    const bool fits = new_sr > 0 && new_sr <= WA_MAX_NEW_SR &&
                      ((int64_t)(WA_TILE - 1) * sr) / new_sr + 1 + 2 * (int64_t)W + 2 <= span_cap;
    if (any && fits) {
        const int64_t kc_lo = j_lo * sr / new_sr, kc_hi = j_hi * sr / new_sr;
        k_lo = kc_lo - W;
        len = (int)(kc_hi - kc_lo + 2 * (int64_t)W + 2);             // <= the full tile's span
    }
    if (!fits) {                                           // a row the launch was not sized for: loud, not out of bounds
        for (int m = m0 + tid; m < m1; m += WA_THREADS) yo[m] = m < p.n_out ? __int_as_float(0x7fc00000) : 0.f;
        return;
    }
    float* span = wa_lds;
    const float* tab = table;
    for (int t = tid; t < len; t += WA_THREADS) span[t] = wa_input(p, xr, b, k_lo + t);
    __syncthreads();

    const int step = new_sr * WA_P;                        // |D| P moves by this much per tap
    const int si = step / q, se = step - si * q;
    const int dq = (WA_THREADS * sr) / new_sr, dr = WA_THREADS * sr - dq * new_sr;     // kc and the remainder per 256 samples
    const float inv_q = 1.0f / (float)q;
    const float s = new_sr < sr ? (float)new_sr / (float)sr : 1.0f;
    bool have = false;
    int64_t kc = 0;
    int rem = 0;
    for (int m = m0 + tid; m < m1; m += WA_THREADS) {
        if (m >= p.n_out) { yo[m] = 0.f; continue; }
        const int64_t j = (int64_t)m + p.shift_post;
        float r = 0.f;
        if (j >= 0 && j < p.n_out) {
            if (!have) {
                kc = j * sr / new_sr;
                rem = (int)(j * sr - kc * new_sr);
                have = true;
            } else {
                kc += dq; rem += dr;
                if (rem >= new_sr) { rem -= new_sr; ++kc; }
            }
            const int a0 = rem * WA_P;                     // D(kc) P, in [0, step)
            const int i0 = a0 / q, e0 = a0 - i0 * q;
            const int t0 = (int)(kc - k_lo);
            // both wings at once, a fixed W - 1 taps each (no wing has more: Z q / new_sr rounded up) so that the loop unrolls and
            // its LDS reads are in flight together; a tap at or beyond the table's end weighs 0
            float accl = 0.f, accr = 0.f;
            int il = i0, el = e0;                          // k = kc, kc - 1, ...
            int ir = si - i0, er = se - e0;                // k = kc + 1, ...: |D| P = step - a0
            if (er < 0) { er += q; --ir; }
            const float* sc = span + t0;
#pragma unroll 2
            for (int w = 0; w < W - 1; ++w) {
                const int cl = min(il, ZP - 1), cr = min(ir, ZP - 1);
                const float l0 = tab[cl], l1 = tab[cl + 1], r0 = tab[cr], r1 = tab[cr + 1];
                const float wl = il < ZP ? fmaf((float)el * inv_q, l1 - l0, l0) : 0.f;
                const float wr = ir < ZP ? fmaf((float)er * inv_q, r1 - r0, r0) : 0.f;
                accl = fmaf(sc[-w], wl, accl);
                accr = fmaf(sc[w + 1], wr, accr);
                il += si; el += se;
                if (el >= q) { el -= q; ++il; }
                ir += si; er += se;
                if (er >= q) { er -= q; ++ir; }
            }
            r = s * (accl + accr);
        }
        float v = p.gain * r;
        if (out_noise) v += wa_noise(p, b, (int64_t)m + p.noise_shift, p.n_out);
        yo[m] = v;
    }
}

// samples of LDS span a tile needs at new_sr (the kernel's own count, at its largest)
int64_t wa_span_cap(int Z, int sr, int new_sr) {
    const int q = sr > new_sr ? sr : new_sr;
    const int64_t W = ((int64_t)Z * q + new_sr - 1) / new_sr + 1;
    return ((int64_t)(WA_TILE - 1) * sr) / new_sr + 1 + 2 * W + 2;
}

}  // namespace

extern "C" int ia_wave_augment_tile(void) { return WA_TILE; }

extern "C" int ia_wave_augment(const float* x, int B, int L_in, float* y, int L_out, const ia_wave_params* params,
                               const float* table, int zero_crossings, int sr, int min_new_sr, ia_stream_t stream) {
    if (!x || !y || !params || x == y || B <= 0 || L_in <= 0 || L_out <= 0 || sr <= 0 || sr > WA_MAX_SR || min_new_sr < 0 ||
        min_new_sr > WA_MAX_NEW_SR)
        return IA_INVALID_VALUE;
    if (!ia_is_aligned(x, 4) || !ia_is_aligned(y, 4) || !ia_is_aligned(params, 4) || !ia_is_aligned(table, 4)) return IA_INVALID_VALUE;
    if (min_new_sr > 0 && (!table || (zero_crossings != 16 && zero_crossings != 64))) return IA_INVALID_VALUE;
    const int tiles = (L_out + WA_TILE - 1) / WA_TILE;
    if ((int64_t)B * tiles > 0x7fffffff) return IA_INVALID_VALUE;
    int64_t span_cap = 0;
    size_t lds = 0;
    if (min_new_sr > 0) {
        span_cap = (wa_span_cap(zero_crossings, sr, min_new_sr) + 3) / 4 * 4;
        const int64_t bytes = span_cap * (int64_t)sizeof(float);
        if (bytes > WA_LDS_BYTES) return IA_UNSUPPORTED;
        lds = (size_t)bytes;
    }
    const dim3 grid((unsigned)(B * tiles)), block(WA_THREADS);
    if (min_new_sr > 0 && zero_crossings == 64) {
        IA_SET_MAX_LDS_ONCE((wave_augment_kernel<64>), lds);
        hipLaunchKernelGGL((wave_augment_kernel<64>), grid, block, lds, (hipStream_t)stream, x, L_in, y, L_out, params, table,
                           sr, (int)span_cap, tiles);
    } else {
        IA_SET_MAX_LDS_ONCE((wave_augment_kernel<16>), lds);
        hipLaunchKernelGGL((wave_augment_kernel<16>), grid, block, lds, (hipStream_t)stream, x, L_in, y, L_out, params, table,
                           sr, (int)span_cap, tiles);
    }
    IA_RETURN_IF_LAUNCH_FAILED();
    return IA_OK;
}
