// Audio front end on the device (include/aptai_hip.h, "audio front end"): batched polyphase resampling of a packed buffer of
// utterances (float32 or int16 PCM) into the zero-padded [B][ld] batch the models take, and the feature extractor's
// zero-mean / unit-variance normalisation over the valid samples.  Both are bandwidth-bound; no atomics, fixed summation order.
#include "common.h"

namespace {

constexpr int FE_THREADS = 256;
constexpr int FE_WAVES = FE_THREADS / 64;

// ---------------------------------------------------------------------------------------------------------------- resampling
// One block produces up to RS_TILE consecutive output samples of one utterance (thread i: n0 + i, n0 + i + 256, ...; a wave
// stores 256 contiguous bytes).
// LDS: the source span of the tile as fp32 (int16 converted while staging), 16-byte global loads on 16-byte boundaries of the
// packed buffer, elements outside [offsets[b], offsets[b+1]) filled with 0.0 and never loaded; the tap table [new][Kc] and
// `first` when they fit.  One output sample is acc = fma(taps[p][j], x[s + j], acc) for j = 0 .. Kc-1 from acc = 0, x = 0
// outside the utterance: the same sequence whether x comes from LDS or (a span that does not cover the sample, a table the host
// did not lay out monotonically) from global memory, whatever the tile, the crop or the neighbours.
constexpr int RS_TILE = 1024;                    // outputs per block; the host shrinks it (in steps of 256) for steep ratios
constexpr int RS_SPAN = 6144;                    // fp32 elements of source per tile held in LDS (24 KiB)
constexpr int RS_TAPS = 8704;                    // fp32 tap entries held in LDS (34 KiB); larger tables are read through L2
constexpr int RS_FIRST = 1024;                   // `first` entries held in LDS with them (4 KiB; 62 KiB in all at most)

__device__ __forceinline__ float src_load(const float* s, long i) { return s[i]; }
__device__ __forceinline__ float src_load(const int16_t* s, long i) { return (float)s[i] * (1.0f / 32768.0f); }

// 16 bytes of source starting at element g (g a multiple of the vector length, the buffer 16-byte aligned) -> fp32 in LDS
__device__ __forceinline__ void stage_vec(const float* s, long g, float* dst) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(s + g);
    dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2]; dst[3] = v[3];
}
__device__ __forceinline__ void stage_vec(const int16_t* s, long g, float* dst) {
    const short8v v = *reinterpret_cast<const short8v*>(s + g);
#pragma unroll
    for (int e = 0; e < 8; ++e) dst[e] = (float)v[e] * (1.0f / 32768.0f);
}

// One tile of row blockIdx.y at the ratio orig -> new_ with its bank (taps, first): the body of both resampling kernels, so a row
// of the per-row-ratio launch runs the instructions the single-ratio launch runs for it.
// TL: the tap table and `first` are staged in LDS (ds_read instead of flat loads on the inner loop)
template <typename SRC, bool TL>
__device__ __forceinline__ void resample_tile(const SRC* __restrict__ src, const long long* __restrict__ offsets,
                                              const float* __restrict__ taps, const int* __restrict__ first, int orig,
                                              int new_, int Kc, int width, const long long* __restrict__ out_start,
                                              float* __restrict__ out, long ld, int ncols, int tile) {
    constexpr int VEC = 16 / (int)sizeof(SRC);
    extern __shared__ __attribute__((aligned(16))) float fe_lds[];           // xs[RS_SPAN] | taps[new * Kc] | first[new] (the last two when staged)
    float* xs = fe_lds;
    float* taps_s = fe_lds + RS_SPAN;
    int* first_s = reinterpret_cast<int*>(taps_s + new_ * Kc);
    const int b = blockIdx.y, tid = threadIdx.x;
    const long off_b = offsets[b], off_e = offsets[b + 1];
    const long len = off_e > off_b ? off_e - off_b : 0;
    const long n_out = ((long)new_ * len + orig - 1) / orig;                 // ceil(new * len / orig)
    long start = out_start ? out_start[b] : 0;
    start = start < 0 ? 0 : start;
    float* orow = out + (long)b * ld;
    const bool copy = orig == new_;

    const long c0 = (long)blockIdx.x * tile;                                // the grid covers ncols: c0 < ncols
    const int cols = ncols - c0 < tile ? (int)(ncols - c0) : tile;
    const long n0 = start + c0;
    if (n0 >= n_out || copy) {                                              // padding only, or the identity ratio: nothing staged (uniform)
        for (int i = tid; i < cols; i += FE_THREADS) {
            const long n = n0 + i;
            orow[c0 + i] = (copy && n < n_out) ? src_load(src, off_b + n) : 0.0f;
        }
        return;
    }
    if (TL) {
        for (int i = tid; i < new_ * Kc; i += FE_THREADS) taps_s[i] = taps[i];
        for (int i = tid; i < new_; i += FE_THREADS) first_s[i] = first[i];
        __syncthreads();
    }
    const float* tp = TL ? taps_s : taps;
    const int* fp = TL ? first_s : first;
    // span of the tile: from the first tap of its first sample to the last tap of its last valid sample, both relative to the
    // utterance's first sample; the LDS copy starts on the 16-byte boundary of the packed buffer at or below it
    const long nl = (n0 + cols < n_out ? n0 + cols : n_out) - 1;
    const long q0 = n0 / new_;
    const int p0 = (int)(n0 - q0 * new_);                                    // per tile; the samples below divide 32-bit numbers
    const long lo = q0 * orig + fp[p0] - width;
    const long hi = (nl / new_) * orig + fp[nl % new_] - width + Kc;        // exclusive
    const long g_lo = (off_b + lo) & ~(long)(VEC - 1);                      // packed-buffer element of xs[0] (floor, also when negative)
    long span = hi + off_b - g_lo;
    span = span < 0 ? 0 : (span > RS_SPAN ? RS_SPAN : span);
    for (long v = (long)tid * VEC; v < span; v += (long)FE_THREADS * VEC) {
        const long g = g_lo + v;
        if (g >= off_b && g + VEC <= off_e) {
            stage_vec(src, g, xs + v);
        } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e) xs[v + e] = (g + e >= off_b && g + e < off_e) ? src_load(src, g + e) : 0.0f;
        }
    }
    __syncthreads();
    const long span_al = (span + VEC - 1) & ~(long)(VEC - 1);                // what the loop above filled (RS_SPAN is a multiple of VEC)
    for (int i = tid; i < cols; i += FE_THREADS) {
        const long n = n0 + i;
        float acc = 0.0f;
        if (n < n_out) {
            const int dq = (p0 + i) / new_, p = (p0 + i) - dq * new_;
            const long q = q0 + dq;
            const long s = q * orig + fp[p] - width;                         // utterance-relative index of tap 0
            const float* trow = tp + (long)p * Kc;
            const long l0 = s + off_b - g_lo;
            if (l0 >= 0 && l0 + Kc <= span_al) {
                const float* xr = xs + l0;
                for (int j = 0; j < Kc; ++j) acc = fmaf(trow[j], xr[j], acc);
            } else {                                                         // taps outside the staged span: the same sequence on global operands
                for (int j = 0; j < Kc; ++j) {
                    const long r = s + j;
                    const float x = (r >= 0 && r < len) ? src_load(src, off_b + r) : 0.0f;
                    acc = fmaf(trow[j], x, acc);
                }
            }
        }
        orow[c0 + i] = acc;
    }
}

template <typename SRC, bool TL>
__global__ __launch_bounds__(FE_THREADS) void resample_kernel(const SRC* __restrict__ src, const long long* __restrict__ offsets,
                                                              const float* __restrict__ taps, const int* __restrict__ first, int orig,
                                                              int new_, int Kc, int width, const long long* __restrict__ out_start,
                                                              float* __restrict__ out, long ld, int ncols, int tile) {
    resample_tile<SRC, TL>(src, offsets, taps, first, orig, new_, Kc, width, out_start, out, ld, ncols, tile);
}

// Per-row ratios: row b runs at entry ratio[b] of `table` (RS_ENTRY int32 words each: orig, new, Kc, width, the offsets of its taps
// and `first` inside the concatenated arrays, two spare words).  blockIdx.y picks the row, so the entry is read with scalar loads and
// every branch on it is uniform.  A bank is staged when it fits both the LDS budget of the single-ratio kernel and what this launch
// reserved behind the source span (lds_bank entries, taps and `first` together); staging never changes a bit.
constexpr int RS_ENTRY = 8;

template <typename SRC>
__global__ __launch_bounds__(FE_THREADS) void resample_multi_kernel(const SRC* __restrict__ src, const long long* __restrict__ offsets,
                                                                    const float* __restrict__ taps, const int* __restrict__ first,
                                                                    const int* __restrict__ table, const int* __restrict__ ratio,
                                                                    int n_ratios, int lds_bank, const long long* __restrict__ out_start,
                                                                    float* __restrict__ out, long ld, int ncols, int tile) {
    int r = ratio[blockIdx.y];
    r = r < 0 ? 0 : (r >= n_ratios ? n_ratios - 1 : r);                      // checked on the host; never an index outside the table
    const int* e = table + r * RS_ENTRY;
    const int orig = e[0], new_ = e[1], Kc = e[2], width = e[3];
    const float* tp = taps + e[4];
    const int* fp = first + e[5];
    const bool staged = orig != new_ && (long)new_ * Kc <= RS_TAPS && new_ <= RS_FIRST && (long)new_ * Kc + new_ <= lds_bank;
    if (staged) resample_tile<SRC, true>(src, offsets, tp, fp, orig, new_, Kc, width, out_start, out, ld, ncols, tile);
    else resample_tile<SRC, false>(src, offsets, tp, fp, orig, new_, Kc, width, out_start, out, ld, ncols, tile);
}

// ---------------------------------------------------------------------------------------------------------------- target warping
// Row r of the launch: a fp64 track (r < R_trk) or an int64 label row, n_in[r] frames -> n_out[r] frames over the same time range.
// Positions are numpy's linspace(0, n_in - 1, n_out): p_i = i * ((n_in - 1) / (n_out - 1)), the last one n_in - 1 itself.  Every
// product is rounded before it is used (fe_rounded), so nothing contracts into an fma and a track is hostlogic.warp_track's bits.
constexpr double WT_IGNORE = -100.0;

__device__ __forceinline__ double fe_rounded(double v) {
    asm volatile("" : "+v"(v));
    return v;
}

__global__ __launch_bounds__(FE_THREADS) void warp_targets_kernel(const double* __restrict__ trk, const long long* __restrict__ lab,
                                                                  int R_trk, long ld_in, int T_in, const long long* __restrict__ n_in_,
                                                                  const long long* __restrict__ n_out_, double* __restrict__ trk_out,
                                                                  long long* __restrict__ lab_out, long ld_out, int T_out) {
    const int r = blockIdx.y;
    const int i = blockIdx.x * FE_THREADS + threadIdx.x;
    if (i >= T_out) return;
    long long ni = n_in_[r], no = n_out_[r];
    const int n_in = ni < 0 ? 0 : (ni > T_in ? T_in : (int)ni);              // nothing outside the row is read or written
    const int n_out = (n_in == 0 || no < 0) ? 0 : (no > T_out ? T_out : (int)no);
    const bool track = r < R_trk;
    if (i >= n_out) {
        if (track) trk_out[(long)r * ld_out + i] = WT_IGNORE;
        else lab_out[(long)(r - R_trk) * ld_out + i] = 0;
        return;
    }
    double p;
    if (n_out == 1) p = 0.0;
    else if (i == n_out - 1) p = (double)(n_in - 1);
    else p = fe_rounded((double)i * ((double)(n_in - 1) / (double)(n_out - 1)));
    if (track) {
        const double* x = trk + (long)r * ld_in;
        double y;
        if (n_in == n_out) {
            y = x[i];
        } else {
            int lo = (int)floor(p);
            const int top = n_in - 2 > 0 ? n_in - 2 : 0;
            lo = lo < 0 ? 0 : (lo > top ? top : lo);
            const int hi = lo + 1 < n_in - 1 ? lo + 1 : n_in - 1;
            const double w = p - (double)lo;
            const double xl = x[lo], xh = x[hi];
            y = xl + fe_rounded(fe_rounded(xh - xl) * w);
            if (xl == WT_IGNORE || (w > 0.0 && xh == WT_IGNORE)) y = WT_IGNORE;
        }
        trk_out[(long)r * ld_out + i] = y;
    } else {
        const long long* x = lab + (long)(r - R_trk) * ld_in;
        int k = (int)floor(p + 0.5);
        k = k > n_in - 1 ? n_in - 1 : (k < 0 ? 0 : k);
        lab_out[(long)(r - R_trk) * ld_out + i] = x[k];
    }
}

// ---------------------------------------------------------------------------------------------------------------- normalisation
// Fixed tree: the caller's lane-strided partial -> xor-shuffle tree inside the wave -> the waves' totals added in wave order.
__device__ __forceinline__ double fe_block_sum(double v, double* slot) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = slot[0];
#pragma unroll
    for (int w = 1; w < FE_WAVES; ++w) s += slot[w];
    __syncthreads();
    return s;
}

constexpr int WN_CHUNK = 8192;                   // samples per block

__device__ __forceinline__ int wn_len(const long long* lens, int b, int ncols) {
    const long long n = lens[b];
    return n < 0 ? 0 : (n > ncols ? ncols : (int)n);
}

// Pass 1, block (chunk, b): sums of d and d*d over the chunk's valid samples, d = x - x[b][0] in fp64.  The shift is a sample of
// the utterance, so |mean d| is of the order of the spread and sum d*d - (sum d)^2 / n does not cancel, whatever the offset.
template <bool VEC4>
__global__ __launch_bounds__(FE_THREADS) void wave_stats_kernel(const float* __restrict__ x, long ld, const long long* __restrict__ lens,
                                                                int ncols, int nchunks, double* __restrict__ part) {
    __shared__ double slot[FE_WAVES];
    const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int n = wn_len(lens, b, ncols);
    const int i0 = c * WN_CHUNK;
    if (i0 >= n) return;                                                    // uniform; pass 2 reads only the chunks below n
    const int i1 = i0 + WN_CHUNK < n ? i0 + WN_CHUNK : n;
    const float* row = x + (long)b * ld;
    const double shift = (double)row[0];
    double s1 = 0.0, s2 = 0.0;
    if (VEC4) {
        const int v1 = i0 + ((i1 - i0) & ~3);
        for (int i = i0 + tid * 4; i < v1; i += FE_THREADS * 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(row + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double d = (double)v[e] - shift;
                s1 += d;
                s2 = fma(d, d, s2);
            }
        }
        if (tid < i1 - v1) {
            const double d = (double)row[v1 + tid] - shift;
            s1 += d;
            s2 = fma(d, d, s2);
        }
    } else {
        for (int i = i0 + tid; i < i1; i += FE_THREADS) {
            const double d = (double)row[i] - shift;
            s1 += d;
            s2 = fma(d, d, s2);
        }
    }
    s1 = fe_block_sum(s1, slot);
    s2 = fe_block_sum(s2, slot);
    if (tid == 0) {
        part[((long)b * nchunks + c) * 2] = s1;
        part[((long)b * nchunks + c) * 2 + 1] = s2;
        if (c == 0) part[(long)gridDim.y * nchunks * 2 + b] = shift;        // pass 2 rewrites x[b][0]: the shift travels with the sums
    }
}

// Pass 2, block (chunk, b): every block adds the utterance's chunk sums in the same order (thread-strided, then the tree), forms
// mean and 1 / sqrt(var + 1e-7) in fp64 and rewrites its chunk: y = fp32((x - mean) * rstd), one rounding.
template <bool VEC4>
__global__ __launch_bounds__(FE_THREADS) void wave_apply_kernel(float* __restrict__ x, long ld, const long long* __restrict__ lens, int ncols,
                                                                int nchunks, const double* __restrict__ part) {
    __shared__ double slot[FE_WAVES];
    const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int n = wn_len(lens, b, ncols);
    const int i0 = c * WN_CHUNK;
    if (i0 >= n) return;
    const int i1 = i0 + WN_CHUNK < n ? i0 + WN_CHUNK : n;
    const int used = (n + WN_CHUNK - 1) / WN_CHUNK;
    double s1 = 0.0, s2 = 0.0;
    for (int k = tid; k < used; k += FE_THREADS) {
        s1 += part[((long)b * nchunks + k) * 2];
        s2 += part[((long)b * nchunks + k) * 2 + 1];
    }
    s1 = fe_block_sum(s1, slot);
    s2 = fe_block_sum(s2, slot);
    float* row = x + (long)b * ld;
    const double shift = part[(long)gridDim.y * nchunks * 2 + b];
    const double md = s1 / (double)n;
    double var = (s2 - s1 * md) / (double)n;
    var = var < 0.0 ? 0.0 : var;
    const double mean = shift + md;
    const double rstd = 1.0 / sqrt(var + 1e-7);
    if (VEC4) {
        const int v1 = i0 + ((i1 - i0) & ~3);
        for (int i = i0 + tid * 4; i < v1; i += FE_THREADS * 4) {
            f32x4 v = *reinterpret_cast<const f32x4*>(row + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (float)(((double)v[e] - mean) * rstd);
            *reinterpret_cast<f32x4*>(row + i) = v;
        }
        if (tid < i1 - v1) row[v1 + tid] = (float)(((double)row[v1 + tid] - mean) * rstd);
    } else {
        for (int i = i0 + tid; i < i1; i += FE_THREADS) row[i] = (float)(((double)row[i] - mean) * rstd);
    }
}

}  // namespace

extern "C" int aptai_resample_batch(const void* src, int src_is_int16, const int64_t* offsets, int64_t B, const float* taps,
                                    const int32_t* first, int64_t orig, int64_t new_, int64_t Kc, int64_t width, const int64_t* out_start,
                                    float* out, int64_t ld, int64_t ncols, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    APTAI_REQUIRE(src && offsets && out, "aptai_resample_batch: null pointer");
    APTAI_REQUIRE(src_is_int16 == 0 || src_is_int16 == 1, "aptai_resample_batch: src_is_int16 must be 0 or 1 (got %d)", src_is_int16);
    APTAI_REQUIRE(B > 0 && B <= 65535 && ncols >= 0 && ncols <= 0x7fffffff && ld >= ncols && ld >= 1,
                  "aptai_resample_batch: bad sizes (B=%ld, ld=%ld, ncols=%ld)", (long)B, (long)ld, (long)ncols);
    APTAI_REQUIRE(orig >= 1 && new_ >= 1 && orig <= 0x7fffffff && new_ <= 0x7fffffff, "aptai_resample_batch: bad ratio %ld -> %ld",
                  (long)orig, (long)new_);
    APTAI_REQUIRE(((uintptr_t)src & 15) == 0, "aptai_resample_batch: the packed source buffer must be 16-byte aligned");
    if (orig != new_) {
        APTAI_REQUIRE(taps && first, "aptai_resample_batch: null filter table");
        APTAI_REQUIRE(Kc >= 1 && width >= 0 && width <= 0x3fffffff && Kc <= APTAI_RESAMPLE_MAX_TABLE,
                      "aptai_resample_batch: bad filter (Kc=%ld, width=%ld)", (long)Kc, (long)width);
        APTAI_REQUIRE(new_ * Kc <= APTAI_RESAMPLE_MAX_TABLE, "aptai_resample_batch: a tap table of %ld x %ld entries exceeds %d",
                      (long)new_, (long)Kc, APTAI_RESAMPLE_MAX_TABLE);
    }
    if (ncols == 0) return APTAI_OK;
    const int taps_in_lds = (orig != new_ && new_ * Kc <= RS_TAPS && new_ <= RS_FIRST) ? 1 : 0;
    // the tile's source span, tile * orig / new + Kc samples (+ 8 of alignment, + 2 of rounding), has to fit RS_SPAN; a sample
    // whose taps do not lie in the staged span is still right (it reads global memory), only slower
    int64_t tile = RS_TILE;
    if (orig != new_) {
        const int64_t fit = (RS_SPAN - Kc - 10) * new_ / orig;
        tile = fit >= RS_TILE ? RS_TILE : (fit < 256 ? 256 : fit / 256 * 256);
    }
    const int64_t tiles = ceil_div(ncols, tile);
    const size_t lds = sizeof(float) * (RS_SPAN + (taps_in_lds ? (size_t)(new_ * Kc + new_) : 0));
    const dim3 grid((unsigned)tiles, (unsigned)B);
#define FE_RESAMPLE(SRC, TL)                                                                                                           \
    APTAI_LAUNCH((resample_kernel<SRC, TL>), grid, dim3(FE_THREADS), lds, stream, (const SRC*)src, (const long long*)offsets, taps, first, \
                 (int)orig, (int)new_, (int)Kc, (int)width, (const long long*)out_start, out, (long)ld, (int)ncols, (int)tile)
    if (src_is_int16) {
        if (taps_in_lds) FE_RESAMPLE(int16_t, true); else FE_RESAMPLE(int16_t, false);
    } else {
        if (taps_in_lds) FE_RESAMPLE(float, true); else FE_RESAMPLE(float, false);
    }
#undef FE_RESAMPLE
    APTAI_CHECK_LAUNCH("resample_kernel");
    return APTAI_OK;
}

extern "C" int aptai_resample_batch_multi(const void* src, int src_is_int16, const int64_t* offsets, int64_t B, const float* taps,
                                          int64_t n_taps, const int32_t* first, int64_t n_first, const int32_t* table,
                                          const int32_t* table_host, int64_t n_ratios, const int32_t* ratio, const int32_t* ratio_host,
                                          const int64_t* out_start, float* out, int64_t ld, int64_t ncols, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    APTAI_REQUIRE(src && offsets && out && table && table_host && ratio && ratio_host, "aptai_resample_batch_multi: null pointer");
    APTAI_REQUIRE(src_is_int16 == 0 || src_is_int16 == 1, "aptai_resample_batch_multi: src_is_int16 must be 0 or 1 (got %d)", src_is_int16);
    APTAI_REQUIRE(B > 0 && B <= 65535 && ncols >= 0 && ncols <= 0x7fffffff && ld >= ncols && ld >= 1,
                  "aptai_resample_batch_multi: bad sizes (B=%ld, ld=%ld, ncols=%ld)", (long)B, (long)ld, (long)ncols);
    APTAI_REQUIRE(n_ratios >= 1 && n_ratios <= APTAI_RESAMPLE_MAX_RATIOS, "aptai_resample_batch_multi: %ld ratios, 1 .. %d expected",
                  (long)n_ratios, APTAI_RESAMPLE_MAX_RATIOS);
    APTAI_REQUIRE(n_taps >= 0 && n_first >= 0 && n_taps <= 0x7fffffff && n_first <= 0x7fffffff,
                  "aptai_resample_batch_multi: bad table sizes (%ld taps, %ld first)", (long)n_taps, (long)n_first);
    APTAI_REQUIRE(((uintptr_t)src & 15) == 0, "aptai_resample_batch_multi: the packed source buffer must be 16-byte aligned");
    bool present[APTAI_RESAMPLE_MAX_RATIOS] = {};
    for (int64_t b = 0; b < B; ++b) {
        APTAI_REQUIRE(ratio_host[b] >= 0 && ratio_host[b] < n_ratios, "aptai_resample_batch_multi: row %ld has ratio index %d, the table has %ld",
                      (long)b, (int)ratio_host[b], (long)n_ratios);
        present[ratio_host[b]] = true;
    }
    // the tile is the smallest fit over the ratios present (the rule of aptai_resample_batch); the LDS behind the source span holds
    // the largest bank among them that fits the budget
    int64_t tile = RS_TILE, lds_bank = 0;
    for (int64_t r = 0; r < n_ratios; ++r) {
        const int32_t* e = table_host + r * RS_ENTRY;
        const int64_t orig = e[0], new_ = e[1], Kc = e[2], width = e[3], t_off = e[4], f_off = e[5];
        APTAI_REQUIRE(orig >= 1 && new_ >= 1, "aptai_resample_batch_multi: entry %ld has the ratio %ld -> %ld", (long)r, (long)orig, (long)new_);
        if (orig == new_) continue;
        APTAI_REQUIRE(taps && first, "aptai_resample_batch_multi: null filter table");
        APTAI_REQUIRE(Kc >= 1 && width >= 0 && width <= 0x3fffffff && Kc <= APTAI_RESAMPLE_MAX_TABLE,
                      "aptai_resample_batch_multi: entry %ld has a bad filter (Kc=%ld, width=%ld)", (long)r, (long)Kc, (long)width);
        APTAI_REQUIRE(new_ * Kc <= APTAI_RESAMPLE_MAX_TABLE, "aptai_resample_batch_multi: entry %ld: a tap table of %ld x %ld entries exceeds %d",
                      (long)r, (long)new_, (long)Kc, APTAI_RESAMPLE_MAX_TABLE);
        APTAI_REQUIRE(t_off >= 0 && f_off >= 0 && t_off + new_ * Kc <= n_taps && f_off + new_ <= n_first,
                      "aptai_resample_batch_multi: entry %ld lies outside the concatenated tables", (long)r);
        if (!present[r]) continue;
        const int64_t fit = (RS_SPAN - Kc - 10) * new_ / orig;
        const int64_t t = fit >= RS_TILE ? RS_TILE : (fit < 256 ? 256 : fit / 256 * 256);
        tile = t < tile ? t : tile;
        if (new_ * Kc <= RS_TAPS && new_ <= RS_FIRST && new_ * Kc + new_ > lds_bank) lds_bank = new_ * Kc + new_;
    }
    if (ncols == 0) return APTAI_OK;
    const int64_t tiles = ceil_div(ncols, tile);
    const size_t lds = sizeof(float) * (size_t)(RS_SPAN + lds_bank);
    const dim3 grid((unsigned)tiles, (unsigned)B);
#define FE_RESAMPLE_MULTI(SRC)                                                                                                          \
    APTAI_LAUNCH((resample_multi_kernel<SRC>), grid, dim3(FE_THREADS), lds, stream, (const SRC*)src, (const long long*)offsets, taps, first, \
                 (const int*)table, (const int*)ratio, (int)n_ratios, (int)lds_bank, (const long long*)out_start, out, (long)ld, (int)ncols, \
                 (int)tile)
    if (src_is_int16) FE_RESAMPLE_MULTI(int16_t); else FE_RESAMPLE_MULTI(float);
#undef FE_RESAMPLE_MULTI
    APTAI_CHECK_LAUNCH("resample_multi_kernel");
    return APTAI_OK;
}

extern "C" int aptai_warp_targets(const double* tracks, int64_t R_trk, const int64_t* labels, int64_t R_lab, int64_t ld_in, int64_t T_in,
                                  const int64_t* n_in, const int64_t* n_out, double* tracks_out, int64_t* labels_out, int64_t ld_out,
                                  int64_t T_out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    APTAI_REQUIRE(R_trk >= 0 && R_lab >= 0 && R_trk + R_lab >= 1 && R_trk + R_lab <= 65535, "aptai_warp_targets: bad row counts (%ld tracks, %ld label rows)",
                  (long)R_trk, (long)R_lab);
    APTAI_REQUIRE(n_in && n_out && (R_trk == 0 || (tracks && tracks_out)) && (R_lab == 0 || (labels && labels_out)),
                  "aptai_warp_targets: null pointer");
    APTAI_REQUIRE(T_in >= 0 && T_out >= 0 && T_in <= 0x7fffffff && T_out <= 0x7fffffff && ld_in >= T_in && ld_out >= T_out,
                  "aptai_warp_targets: bad sizes (T_in=%ld, ld_in=%ld, T_out=%ld, ld_out=%ld)", (long)T_in, (long)ld_in, (long)T_out, (long)ld_out);
    if (T_out == 0) return APTAI_OK;
    const dim3 grid((unsigned)ceil_div(T_out, FE_THREADS), (unsigned)(R_trk + R_lab));
    APTAI_LAUNCH(warp_targets_kernel, grid, dim3(FE_THREADS), 0, stream, tracks, (const long long*)labels, (int)R_trk, (long)ld_in, (int)T_in,
                 (const long long*)n_in, (const long long*)n_out, tracks_out, (long long*)labels_out, (long)ld_out, (int)T_out);
    APTAI_CHECK_LAUNCH("warp_targets_kernel");
    return APTAI_OK;
}

extern "C" int64_t aptai_wave_normalize_workspace_bytes(int64_t B, int64_t ncols) {
    if (B <= 0 || ncols <= 0) return 0;
    return B * (ceil_div(ncols, WN_CHUNK) * 2 + 1) * (int64_t)sizeof(double);   // {sum d, sum d*d} per chunk, the shift per utterance
}

extern "C" int aptai_wave_normalize(float* x, int64_t ld, const int64_t* lens, int64_t B, int64_t ncols, void* workspace, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    APTAI_REQUIRE(x && lens, "aptai_wave_normalize: null pointer");
    APTAI_REQUIRE(B > 0 && B <= 65535 && ncols >= 0 && ncols <= 0x7fffffff && ld >= ncols && ld >= 1,
                  "aptai_wave_normalize: bad sizes (B=%ld, ld=%ld, ncols=%ld)", (long)B, (long)ld, (long)ncols);
    if (ncols == 0) return APTAI_OK;
    APTAI_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0, "aptai_wave_normalize: workspace missing or not 8-byte aligned");
    const int nchunks = (int)ceil_div(ncols, WN_CHUNK);
    const dim3 grid((unsigned)nchunks, (unsigned)B);
    const bool vec4 = (ld % 4 == 0) && (((uintptr_t)x & 15) == 0);
    double* part = (double*)workspace;
    if (vec4) {
        APTAI_LAUNCH(wave_stats_kernel<true>, grid, dim3(FE_THREADS), 0, stream, x, (long)ld, (const long long*)lens, (int)ncols, nchunks, part);
        APTAI_CHECK_LAUNCH("wave_stats_kernel");
        APTAI_LAUNCH(wave_apply_kernel<true>, grid, dim3(FE_THREADS), 0, stream, x, (long)ld, (const long long*)lens, (int)ncols, nchunks, part);
    } else {
        APTAI_LAUNCH(wave_stats_kernel<false>, grid, dim3(FE_THREADS), 0, stream, x, (long)ld, (const long long*)lens, (int)ncols, nchunks, part);
        APTAI_CHECK_LAUNCH("wave_stats_kernel");
        APTAI_LAUNCH(wave_apply_kernel<false>, grid, dim3(FE_THREADS), 0, stream, x, (long)ld, (const long long*)lens, (int)ncols, nchunks, part);
    }
    APTAI_CHECK_LAUNCH("wave_apply_kernel");
    return APTAI_OK;
}
