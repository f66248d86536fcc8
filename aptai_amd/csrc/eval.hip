// Evaluation metrics of the reference's validate()/test() on the device (include/aptai_hip.h, "evaluation metrics"): per-track
// RMSE / Pearson r, frame accuracy counts, boundary hit counts, run collapse and Levenshtein distance.  Every kernel is a few
// thousand operations per utterance: latency-bound, one block (or one wave) per utterance, no atomics, fixed reduction order.
#include "common.h"

// The library is built with -ffp-contract=fast: the fp64 sums of products below accumulate with fused multiply-adds (one rounding
// per term instead of two, so inside the per-term error bound the tests derive for separately rounded operations).  The boundary
// counts involve no product: subtraction, abs and compare are numpy's, bit for bit.

namespace {

constexpr int EVAL_THREADS = 256;
constexpr int EVAL_WAVES = EVAL_THREADS / 64;

// Fixed tree: the caller's lane-strided partial -> xor-shuffle tree inside the wave -> the waves' totals added in wave order.
// Every thread returns the same bits.  `slot` is EVAL_WAVES doubles of LDS owned by this call.
__device__ __forceinline__ double block_sum_f64(double v, double* slot) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = slot[0];
#pragma unroll
    for (int w = 1; w < EVAL_WAVES; ++w) s += slot[w];
    __syncthreads();
    return s;
}
__device__ __forceinline__ int block_sum_i32(int v, int* slot) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = slot[0];
#pragma unroll
    for (int w = 1; w < EVAL_WAVES; ++w) s += slot[w];
    __syncthreads();
    return s;
}

// ---- per-track RMSE and Pearson r.  Block (c, b); fp32 inputs widened to fp64 on load, frames >= lens[b] never loaded.
// Pass 1: sum x, sum y, sum (x-y)^2 and "differs from frame 0" flags.  Pass 2 (scipy's two-pass form): centred sums.
__global__ __launch_bounds__(EVAL_THREADS) void eval_tv_scores_kernel(const float* __restrict__ gt, long ldg, long rows_g,
                                                                      const float* __restrict__ pred, long ldp, long rows_p,
                                                                      const int* __restrict__ lens, int max_len, int C,
                                                                      double* __restrict__ rmse, double* __restrict__ pcc) {
    __shared__ double slot[EVAL_WAVES];
    __shared__ int islot[EVAL_WAVES];
    const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    int T = lens[b];
    T = T < 0 ? 0 : (T > max_len ? max_len : T);
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    if (T == 0) {
        if (tid == 0) { rmse[(long)b * C + c] = nan; pcc[(long)b * C + c] = nan; }
        return;
    }
    const float* g = gt + (long)b * rows_g * ldg + c;
    const float* p = pred + (long)b * rows_p * ldp + c;
    const double x0 = (double)g[0], y0 = (double)p[0];
    double sx = 0.0, sy = 0.0, sd = 0.0;
    int varies = 0;                                      // bit 0: x is not constant, bit 1: y is not constant
    for (int t = tid; t < T; t += EVAL_THREADS) {
        const double x = (double)g[(long)t * ldg], y = (double)p[(long)t * ldp];
        const double d = x - y;
        sx += x; sy += y; sd += d * d;
        varies |= (x != x0 ? 1 : 0) | (y != y0 ? 2 : 0);
    }
    sx = block_sum_f64(sx, slot);
    sy = block_sum_f64(sy, slot);
    sd = block_sum_f64(sd, slot);
    const int vx = block_sum_i32(varies & 1, islot), vy = block_sum_i32((varies >> 1) & 1, islot);
    const double mx = sx / (double)T, my = sy / (double)T;
    double sxy = 0.0, sxx = 0.0, syy = 0.0;
    for (int t = tid; t < T; t += EVAL_THREADS) {
        const double xm = (double)g[(long)t * ldg] - mx, ym = (double)p[(long)t * ldp] - my;
        sxy += xm * ym; sxx += xm * xm; syy += ym * ym;
    }
    sxy = block_sum_f64(sxy, slot);
    sxx = block_sum_f64(sxx, slot);
    syy = block_sum_f64(syy, slot);
    if (tid == 0) {
        rmse[(long)b * C + c] = sqrt(sd / (double)T);
        double r = nan;                                  // a constant track has no correlation (scipy: NaN)
        if (vx > 0 && vy > 0) {
            r = sxy / sqrt(sxx * syy);
            r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);   // comparisons are false for NaN: it passes through
        }
        pcc[(long)b * C + c] = r;
    }
}

// ---- {frames, frames equal} per utterance
__global__ __launch_bounds__(EVAL_THREADS) void eval_frame_scores_kernel(const long long* __restrict__ gt, long ldg,
                                                                         const long long* __restrict__ pred, long ldp,
                                                                         const int* __restrict__ lens, int max_len, int* __restrict__ out) {
    __shared__ int islot[EVAL_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    int T = lens[b];
    T = T < 0 ? 0 : (T > max_len ? max_len : T);
    int eq = 0;
    for (int t = tid; t < T; t += EVAL_THREADS) eq += gt[(long)b * ldg + t] == pred[(long)b * ldp + t] ? 1 : 0;
    eq = block_sum_i32(eq, islot);
    if (tid == 0) { out[2 * b] = T; out[2 * b + 1] = eq; }
}

// ---- boundary hits: #{own_j : min_i |other_i - own_j| <= tol}.  Each thread owns one element per tile of EVAL_THREADS; the
// other side passes through LDS in chunks.  |a - b| is the same fp64 value as |b - a|, so one routine serves both counts.
// The minimum keeps a NaN once met, like numpy's min.
constexpr int BND_CHUNK = 1024;
__device__ int boundary_side(const double* __restrict__ own, int n_own, const double* __restrict__ other, int n_other, double tol,
                             double* stage, int* islot) {
    int hits = 0;
    for (int j0 = 0; j0 < n_own; j0 += EVAL_THREADS) {
        const int j = j0 + threadIdx.x;
        const double v = j < n_own ? own[j] : 0.0;
        double m = __longlong_as_double(0x7ff0000000000000LL);           // +inf
        for (int i0 = 0; i0 < n_other; i0 += BND_CHUNK) {
            const int n = n_other - i0 < BND_CHUNK ? n_other - i0 : BND_CHUNK;
            __syncthreads();
            for (int i = threadIdx.x; i < n; i += EVAL_THREADS) stage[i] = other[i0 + i];
            __syncthreads();
            for (int i = 0; i < n; ++i) {
                const double d = fabs(stage[i] - v);
                m = (d < m || d != d) ? d : m;
            }
        }
        hits += (j < n_own && m <= tol) ? 1 : 0;
    }
    return block_sum_i32(hits, islot);
}
__global__ __launch_bounds__(EVAL_THREADS) void eval_boundary_counts_kernel(const double* __restrict__ y, long ldy, const int* __restrict__ ny,
                                                                            const double* __restrict__ yhat, long ldh, const int* __restrict__ nh,
                                                                            double tol, int* __restrict__ out) {
    __shared__ double stage[BND_CHUNK];
    __shared__ int islot[EVAL_WAVES];
    const int b = blockIdx.x;
    int n_y = ny[b], n_h = nh[b];
    n_y = n_y < 0 ? 0 : (n_y > ldy ? (int)ldy : n_y);
    n_h = n_h < 0 ? 0 : (n_h > ldh ? (int)ldh : n_h);
    int pc = 0, rc = 0;
    if (n_y > 0 && n_h > 0) {                             // uniform per block
        pc = boundary_side(yhat + (long)b * ldh, n_h, y + (long)b * ldy, n_y, tol, stage, islot);
        rc = boundary_side(y + (long)b * ldy, n_y, yhat + (long)b * ldh, n_h, tol, stage, islot);
    }
    if (threadIdx.x == 0) { out[2 * b] = pc; out[2 * b + 1] = rc; }
}

// ---- collapse runs of equal labels (no argmax, no blank): the ballot + prefix-popcount compaction of ctc_greedy_decode_kernel
__global__ __launch_bounds__(64) void eval_collapse_runs_kernel(const long long* __restrict__ x, long ld, const int* __restrict__ lens,
                                                                int* __restrict__ out, int ldo, int* __restrict__ n_out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int T = lens[b];
    T = T < 0 ? 0 : (T > ld ? (int)ld : T);
    for (int l = lane; l < ldo; l += 64) out[(long)b * ldo + l] = 0;
    int count = 0;
    long long carry = 0;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        const long long v = t < T ? x[(long)b * ld + t] : 0;
        long long prev = __shfl_up(v, 1, 64);
        if (lane == 0) prev = carry;
        const bool keep = t < T && (t == 0 || v != prev);
        const unsigned long long m = __ballot(keep);
        const int pos = count + __popcll(m & ((1ull << lane) - 1ull));
        if (keep && pos < ldo) out[(long)b * ldo + pos] = (int)v;
        count += __popcll(m);
        carry = __shfl(v, 63, 64);
    }
    if (lane == 0) n_out[b] = count;
}

// ---- Levenshtein distance, one wave per pair.  Lane l owns rows l*NS+1 .. l*NS+NS of the DP table (symbols of `a`) and keeps
// the column it last finished in registers.  At step s lane l does column j = s - l (b[j]), so the cell above its first row
// (row l*NS, column j) is what lane l-1 finished one step earlier: one shuffle per step; the diagonal is the previous step's
// shuffled value.  Lane 0's boundary row is D[0][j+1] = j+1.  b's symbols travel down the lanes the same way: lane 0 draws
// b[s] from a 64-symbol register chunk, every other lane takes its neighbour's previous symbol.
template <int NS>
__global__ __launch_bounds__(64) void eval_edit_distance_kernel(const int* __restrict__ a, long lda, const int* __restrict__ a_lens,
                                                                const int* __restrict__ bsym, long ldb, const int* __restrict__ b_lens,
                                                                int* __restrict__ dist) {
    const int p = blockIdx.x, lane = threadIdx.x;
    int na = a_lens[p], nb = b_lens[p];
    na = na < 0 ? 0 : (na > lda ? (int)lda : na);
    nb = nb < 0 ? 0 : (nb > ldb ? (int)ldb : nb);
    if (na > 64 * NS) na = 64 * NS;                       // the entry point refuses lda > 64 * NS_max; unreachable
    if (na == 0 || nb == 0) {
        if (lane == 0) dist[p] = na + nb;
        return;
    }
    const int* ar = a + (long)p * lda;
    const int* br = bsym + (long)p * ldb;
    int sym[NS], col[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const int i = lane * NS + k;                      // 0-based symbol index, DP row i + 1
        sym[k] = i < na ? ar[i] : 0;
        col[k] = i + 1;                                   // D[i+1][0]
    }
    int top_prev = lane * NS;                             // D[lane*NS][0]
    int mysym = 0, chunk = 0;
    const int steps = nb + 63;
    for (int s = 0; s < steps; ++s) {
        if ((s & 63) == 0) chunk = s + lane < nb ? br[s + lane] : 0;
        const int head = __shfl(chunk, s & 63, 64);
        const int from_up = __shfl_up(mysym, 1, 64);
        mysym = lane == 0 ? head : from_up;
        int top = __shfl_up(col[NS - 1], 1, 64);
        const int j = s - lane;
        if (lane == 0) top = j + 1;
        if (j >= 0 && j < nb) {
            int diag = top_prev, up = top;
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                const int left = col[k];
                int v = min(left, up) + 1;
                v = min(v, diag + (sym[k] != mysym ? 1 : 0));
                diag = left;
                up = v;
                col[k] = v;
            }
            top_prev = top;
        }
    }
    const int owner = (na - 1) / NS, kk = (na - 1) % NS;
    int res = 0;
#pragma unroll
    for (int k = 0; k < NS; ++k) res = k == kk ? col[k] : res;
    res = __shfl(res, owner, 64);
    if (lane == 0) dist[p] = res;
}

template <int NS>
void launch_edit(const int32_t* a, int64_t lda, const int32_t* a_lens, const int32_t* b, int64_t ldb, const int32_t* b_lens,
                 int32_t* dist, int64_t B, hipStream_t stream) {
    APTAI_LAUNCH(eval_edit_distance_kernel<NS>, dim3((unsigned)B), dim3(64), 0, stream, a, (long)lda, a_lens, b, (long)ldb, b_lens, dist);
}

}  // namespace

extern "C" int aptai_eval_tv_scores(const float* gt, int64_t ldg, int64_t rows_g, const float* pred, int64_t ldp, int64_t rows_p,
                                    const int32_t* lens, int64_t B, int64_t max_len, int64_t C, double* rmse, double* pcc, void* stream) {
    APTAI_REQUIRE(gt && pred && lens && rmse && pcc, "aptai_eval_tv_scores: null pointer");
    APTAI_REQUIRE(B > 0 && B <= 65535 && C > 0 && ldg >= C && ldp >= C && max_len >= 0 && max_len <= 0x7fffffff && rows_g >= max_len &&
                      rows_p >= max_len,
                  "aptai_eval_tv_scores: bad sizes (B=%ld, C=%ld, pitches %ld / %ld, rows %ld / %ld, max_len=%ld)", (long)B, (long)C,
                  (long)ldg, (long)ldp, (long)rows_g, (long)rows_p, (long)max_len);
    APTAI_LAUNCH(eval_tv_scores_kernel, dim3((unsigned)C, (unsigned)B), dim3(EVAL_THREADS), 0, (hipStream_t)stream, gt, (long)ldg,
                 (long)rows_g, pred, (long)ldp, (long)rows_p, lens, (int)max_len, (int)C, rmse, pcc);
    APTAI_CHECK_LAUNCH("eval_tv_scores_kernel");
    return APTAI_OK;
}

extern "C" int aptai_eval_frame_scores(const int64_t* gt, int64_t ldg, const int64_t* pred, int64_t ldp, const int32_t* lens, int64_t B,
                                       int64_t max_len, int32_t* counts, void* stream) {
    APTAI_REQUIRE(gt && pred && lens && counts, "aptai_eval_frame_scores: null pointer");
    APTAI_REQUIRE(B > 0 && max_len >= 0 && max_len <= 0x7fffffff && ldg >= max_len && ldp >= max_len,
                  "aptai_eval_frame_scores: bad sizes (B=%ld, pitches %ld / %ld, max_len=%ld)", (long)B, (long)ldg, (long)ldp, (long)max_len);
    APTAI_LAUNCH(eval_frame_scores_kernel, dim3((unsigned)B), dim3(EVAL_THREADS), 0, (hipStream_t)stream, (const long long*)gt, (long)ldg,
                 (const long long*)pred, (long)ldp, lens, (int)max_len, counts);
    APTAI_CHECK_LAUNCH("eval_frame_scores_kernel");
    return APTAI_OK;
}

extern "C" int aptai_eval_boundary_counts(const double* y, int64_t ldy, const int32_t* ny, const double* yhat, int64_t ldh,
                                          const int32_t* nh, double tolerance, int64_t B, int32_t* counts, void* stream) {
    APTAI_REQUIRE(y && yhat && ny && nh && counts, "aptai_eval_boundary_counts: null pointer");
    APTAI_REQUIRE(B > 0 && ldy >= 1 && ldh >= 1 && ldy <= 0x7fffffff && ldh <= 0x7fffffff,
                  "aptai_eval_boundary_counts: bad sizes (B=%ld, pitches %ld / %ld)", (long)B, (long)ldy, (long)ldh);
    APTAI_LAUNCH(eval_boundary_counts_kernel, dim3((unsigned)B), dim3(EVAL_THREADS), 0, (hipStream_t)stream, y, (long)ldy, ny, yhat,
                 (long)ldh, nh, tolerance, counts);
    APTAI_CHECK_LAUNCH("eval_boundary_counts_kernel");
    return APTAI_OK;
}

extern "C" int aptai_eval_collapse_runs(const int64_t* x, int64_t ld, const int32_t* lens, int64_t B, int32_t* out, int64_t ldo,
                                        int32_t* n_out, void* stream) {
    APTAI_REQUIRE(x && lens && out && n_out, "aptai_eval_collapse_runs: null pointer");
    APTAI_REQUIRE(B > 0 && ld >= 1 && ld <= 0x7fffffff && ldo >= 1 && ldo <= 0x7fffffff,
                  "aptai_eval_collapse_runs: bad sizes (B=%ld, pitches %ld / %ld)", (long)B, (long)ld, (long)ldo);
    APTAI_LAUNCH(eval_collapse_runs_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, (const long long*)x, (long)ld, lens, out,
                 (int)ldo, n_out);
    APTAI_CHECK_LAUNCH("eval_collapse_runs_kernel");
    return APTAI_OK;
}

extern "C" int aptai_eval_edit_distance(const int32_t* a, int64_t lda, const int32_t* a_lens, const int32_t* b, int64_t ldb,
                                        const int32_t* b_lens, int64_t B, int32_t* dist, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    APTAI_REQUIRE(a && b && a_lens && b_lens && dist, "aptai_eval_edit_distance: null pointer");
    APTAI_REQUIRE(B > 0 && lda >= 1 && ldb >= 1 && ldb <= 0x7fffffff, "aptai_eval_edit_distance: bad sizes (B=%ld, pitches %ld / %ld)",
                  (long)B, (long)lda, (long)ldb);
    APTAI_REQUIRE(lda <= APTAI_EVAL_EDIT_MAX_LANE_SIDE || ldb <= APTAI_EVAL_EDIT_MAX_LANE_SIDE,
                  "aptai_eval_edit_distance: sequences of up to %ld and %ld symbols: one side must fit %d (the side kept in registers)",
                  (long)lda, (long)ldb, APTAI_EVAL_EDIT_MAX_LANE_SIDE);
    APTAI_REQUIRE(lda <= APTAI_EVAL_EDIT_MAX_LANE_SIDE,
                  "aptai_eval_edit_distance: `a` is kept in registers and holds at most %d symbols (got %ld, `b` has %ld): swap the sides, "
                  "the distance is symmetric", APTAI_EVAL_EDIT_MAX_LANE_SIDE, (long)lda, (long)ldb);
    const int ns = (int)((lda + 63) / 64);
    if (ns <= 1) launch_edit<1>(a, lda, a_lens, b, ldb, b_lens, dist, B, stream);
    else if (ns <= 4) launch_edit<4>(a, lda, a_lens, b, ldb, b_lens, dist, B, stream);
    else if (ns <= 8) launch_edit<8>(a, lda, a_lens, b, ldb, b_lens, dist, B, stream);
    else if (ns <= 16) launch_edit<16>(a, lda, a_lens, b, ldb, b_lens, dist, B, stream);
    else launch_edit<32>(a, lda, a_lens, b, ldb, b_lens, dist, B, stream);
    APTAI_CHECK_LAUNCH("eval_edit_distance_kernel");
    return APTAI_OK;
}
