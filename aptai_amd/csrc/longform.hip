// Long recordings (include/aptai_hip.h, "long recordings"): the windows of hostlogic.long_form_plan cut out of a packed buffer of
// recordings into the zero-padded batch the encoder takes, and the per-window results stitched back into one row of frames per
// recording with the seam rule of hostlogic.long_form_stitch.  Both stream a few MB at most; no atomics, no LDS, no dependence on
// the launch geometry: equal inputs give equal bits.
#include "common.h"

namespace {

constexpr int LF_THREADS = 256;
constexpr int LF_WAVES = LF_THREADS / 64;
constexpr int LF_MAX_C = 256;                    // channels per frame: four per lane at most

// ---------------------------------------------------------------------------------------------------------------- window gather
// Block (x, y): columns 4 * (x * 256 + tid) .. + 3 of output row y = window first + y.  Every source index is checked against the
// window's own span, and the span against the packed buffer, before it is read; the row's padding is written as 0.0.
// VEC: the output rows are 16-byte aligned (base and pitch), so a thread's four columns go out in one store.
template <bool VEC>
__global__ __launch_bounds__(LF_THREADS) void window_gather_kernel(const float* __restrict__ src, long n_src,
                                                                   const long long* __restrict__ table, long first, float* __restrict__ out,
                                                                   long ld, long S, long long* __restrict__ lens_out) {
    const long row = blockIdx.y;
    const long long* e = table + (first + row) * 3;
    // window = src[off + start .. off + start + count), cut to what the packed buffer holds
    const bool inside = e[0] >= 0 && e[0] <= n_src && e[1] >= 0 && e[1] <= n_src - e[0];
    const long base = inside ? (long)(e[0] + e[1]) : 0;
    long count = inside ? (long)e[2] : 0;
    if (count > n_src - base) count = n_src - base;
    if (count > S) count = S;
    if (count < 0) count = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) lens_out[row] = count;
    const long c0 = 4 * ((long)blockIdx.x * LF_THREADS + threadIdx.x);
    if (c0 >= S) return;
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = c0 + i < count ? src[base + c0 + i] : 0.0f;
    float* o = out + row * ld + c0;
    if (VEC && c0 + 4 <= S) {
        *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (c0 + i < S) o[i] = v[i];
    }
}

// ---------------------------------------------------------------------------------------------------------------- stitch
// One wave per output frame t of recording blockIdx.y, lane l holds channels l, l + 64, l + 128, l + 192.  The covering windows
// follow from t alone: k = min(t / hop, K) always covers it at row j = t - k hop, and k - 1 does too iff j < overlap = W - hop
// (2 hop >= W: never a third).  In the overlap ramp[j] picks x0 (window k - 1), x1 (window k) or the three-operation blend.
__global__ __launch_bounds__(LF_THREADS) void stitch_windows_kernel(const float* __restrict__ x, long ldx, long rows_per_window, long n_windows,
                                                                    const long long* __restrict__ rec, long max_frames, int W, int hop,
                                                                    const float* __restrict__ ramp, int C, float* __restrict__ out, long ldo,
                                                                    long out_rows, long long* __restrict__ argmax) {
    const int lane = threadIdx.x & 63;
    const long t = (long)blockIdx.x * LF_WAVES + (threadIdx.x >> 6);
    const long long* e = rec + (long)blockIdx.y * 3;
    const long w0 = (long)e[0], F = (long)e[1], o0 = (long)e[2];
    if (t >= F) return;                                                            // wave-uniform
    const long K = F <= W ? 0 : (F - W + hop - 1) / hop;
    // a table that points outside the buffers it describes produces nothing
    if (F > max_frames || w0 < 0 || w0 + K >= n_windows || o0 < 0 || o0 + F > out_rows) return;
    long k = t / hop;
    if (k > K) k = K;
    const long j = t - k * hop;                                                    // < frames of window k <= min(W, max_frames) <= rows_per_window
    const bool two = k > 0 && j < W - hop;
    const float r = two ? ramp[j] : 1.0f;
    const float* x1 = x + ((w0 + k) * rows_per_window + j) * ldx;
    const float* x0 = two ? x + ((w0 + k - 1) * rows_per_window + j + hop) * ldx : x1;
    float* orow = out + (o0 + t) * ldo;
    float best = 0.0f;
    int besti = C;                                                                 // lanes without a channel lose every comparison
#pragma unroll
    for (int i = 0; i < LF_MAX_C / 64; ++i) {
        const int c = lane + 64 * i;
        if (c < C) {
            float v;
            if (r >= 1.0f) {
                v = x1[c];
            } else if (r <= 0.0f) {
                v = x0[c];
            } else {
                // the build contracts a * b + c whatever the source says and the __f*_rn spellings are plain operators here: the
                // empty asm makes the rounded product opaque, so the add cannot absorb the multiply (ema_one, csrc/optim.hip)
                const float a = x0[c];
                float s = __fmul_rn(r, __fsub_rn(x1[c], a));
                asm volatile("" : "+v"(s));
                v = __fadd_rn(a, s);
            }
            orow[c] = v;
            if (besti == C || v > best) { best = v; besti = c; }                   // c ascending: the first maximum stays
        }
    }
    if (argmax == nullptr) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(besti, o, 64);
        if (oi < C && (besti == C || ov > best || (ov == best && oi < besti))) { best = ov; besti = oi; }
    }
    if (lane == 0) argmax[o0 + t] = besti;
}

}  // namespace

extern "C" int aptai_window_gather(const float* src, int64_t n_src, const int64_t* table, int64_t n_windows, int64_t first, int64_t rows,
                                   float* out, int64_t ld, int64_t S, int64_t* lens_out, void* stream) {
    APTAI_REQUIRE(src && table && out && lens_out && n_src > 0 && S > 0 && ld >= S, "aptai_window_gather: bad arguments");
    APTAI_REQUIRE(rows > 0 && rows <= 65535 && first >= 0 && first + rows <= n_windows,
                  "aptai_window_gather: windows %ld .. %ld of a table of %ld (at most 65535 rows per launch)", (long)first,
                  (long)(first + rows), (long)n_windows);
    const dim3 grid((unsigned)ceil_div(S, 4 * LF_THREADS), (unsigned)rows);
    const bool vec = ((uintptr_t)out % 16 == 0) && ld % 4 == 0;
    if (vec)
        APTAI_LAUNCH(window_gather_kernel<true>, grid, dim3(LF_THREADS), 0, (hipStream_t)stream, src, (long)n_src,
                     (const long long*)table, (long)first, out, (long)ld, (long)S, (long long*)lens_out);
    else
        APTAI_LAUNCH(window_gather_kernel<false>, grid, dim3(LF_THREADS), 0, (hipStream_t)stream, src, (long)n_src,
                     (const long long*)table, (long)first, out, (long)ld, (long)S, (long long*)lens_out);
    APTAI_CHECK_LAUNCH("window_gather_kernel");
    return APTAI_OK;
}

extern "C" int aptai_stitch_windows(const float* x, int64_t ldx, int64_t rows_per_window, int64_t n_windows, const int64_t* rec,
                                    int64_t n_rec, int64_t max_frames, int64_t window_frames, int64_t hop_frames, const float* ramp,
                                    int64_t C, float* out, int64_t ldo, int64_t out_rows, int64_t* argmax, void* stream) {
    APTAI_REQUIRE(x && rec && out && n_windows > 0 && n_rec > 0 && n_rec <= 65535 && max_frames > 0 && out_rows > 0,
                  "aptai_stitch_windows: bad arguments");
    APTAI_REQUIRE(C > 0 && C <= LF_MAX_C && ldx >= C && ldo >= C, "aptai_stitch_windows: 1 .. %d channels within both pitches (C = %ld)",
                  LF_MAX_C, (long)C);
    APTAI_REQUIRE(window_frames > 0 && hop_frames > 0 && hop_frames <= window_frames && 2 * hop_frames >= window_frames &&
                      window_frames < (1 << 30),
                  "aptai_stitch_windows: hop_frames (%ld) must lie in [window_frames / 2, window_frames] (window_frames = %ld): a frame is "
                  "covered by one or two windows", (long)hop_frames, (long)window_frames);
    APTAI_REQUIRE(rows_per_window >= (max_frames < window_frames ? max_frames : window_frames),
                  "aptai_stitch_windows: a window of up to %ld frames does not fit %ld rows",
                  (long)(max_frames < window_frames ? max_frames : window_frames), (long)rows_per_window);
    APTAI_REQUIRE(ramp || hop_frames == window_frames || max_frames <= window_frames, "aptai_stitch_windows: overlapping windows need the ramp");
    APTAI_LAUNCH(stitch_windows_kernel, dim3((unsigned)ceil_div(max_frames, LF_WAVES), (unsigned)n_rec), dim3(LF_THREADS), 0,
                 (hipStream_t)stream, x, (long)ldx, (long)rows_per_window, (long)n_windows, (const long long*)rec, (long)max_frames,
                 (int)window_frames, (int)hop_frames, ramp, (int)C, out, (long)ldo, (long)out_rows, (long long*)argmax);
    APTAI_CHECK_LAUNCH("stitch_windows_kernel");
    return APTAI_OK;
}
