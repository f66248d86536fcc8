// CTC negative log-likelihood, forward (alpha) and backward (beta + gradient w.r.t. the LOGITS), gfx950.
// Replaces log_softmax + F.ctc_loss at models/w2v2_pr.py:59,73-81 (blank 0, 'mean', zero_infinity) and the
// per-sample nn.CTCLoss loop of ForwardSumLoss (models/modules.py:99-116: per-sample vocabulary, targets 1..N).
//
// The T-step recursions are inherently sequential, so everything that is NOT sequential is taken out of them:
//   1. ctc_lpe_kernel    (parallel, one wave per frame): log-softmax of every frame; the (T,B,V) log_probs output; and
//                         lpe[b][t][s] = log p_t(ext_s), the only values the recursions read (2L+1 per frame instead of V);
//   2. ctc_recur_kernel  (one wave per utterance and direction; alpha and beta run SIDE BY SIDE in one launch): states in
//                         registers (NS consecutive states per lane, neighbours by one lane shuffle), lpe rows prefetched four
//                         frames ahead so no step waits for memory; ~150 cycles per frame instead of two barriers, a
//                         dependent global load and a log-softmax per frame (2.6 us per frame before: rocprofv3, round 2);
//   3. ctc_grad_kernel   (parallel, one wave per frame): state occupancies exp(alpha + beta - lpe + nll) scattered to their
//                         labels in LDS, gradient row = scale * (softmax - occupancy).
// alpha | beta | lpe live in one caller workspace (3 x B*T*S fp32: 12 MB at B=16, T=499, L<=60).  fp32 like the reference.
#include "common.h"

namespace {

constexpr int MAXV = 256;
#define NEG_INF (-INFINITY)

__device__ __forceinline__ float lse2(float a, float b) {
    const float m = fmaxf(a, b);
    if (m == NEG_INF) return NEG_INF;
    return m + __logf(__expf(a - m) + __expf(b - m));
}
__device__ __forceinline__ float lse3(float a, float b, float c) {
    const float m = fmaxf(a, fmaxf(b, c));
    if (m == NEG_INF) return NEG_INF;
    return m + __logf(__expf(a - m) + __expf(b - m) + __expf(c - m));
}

struct CtcArgs {
    const float* logits; long ldl; long rows_per_b;
    const int* targets; long ldt;
    const int* input_lens; const int* target_lens; const int* vocab_sizes;
    int B, T, V, blank, S_max;
    float* log_probs;      // (T,B,V) or null
    float* alpha;          // [B][T][S_max]
    float* nll;            // [B]  (inf when infeasible)
};

// ---- 1. per-frame log-softmax, (T,B,V) output, lpe gather.  grid = ceil(B*T/4) blocks of 4 waves, one frame per wave.
__global__ __launch_bounds__(256) void ctc_lpe_kernel(CtcArgs a, float* __restrict__ lpe) {
    __shared__ float lps[4][MAXV];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long f = (long)blockIdx.x * 4 + wave;
    if (f >= (long)a.B * a.T) return;
    const int b = (int)(f / a.T), t = (int)(f % a.T);
    const int Vb = a.vocab_sizes ? a.vocab_sizes[b] : a.V;
    const float* row = a.logits + ((long)b * a.rows_per_b + t) * a.ldl;
    float x[MAXV / 64];
    float mx = NEG_INF;
#pragma unroll
    for (int j = 0; j < MAXV / 64; ++j) {
        const int v = j * 64 + lane;
        x[j] = v < Vb ? row[v] : NEG_INF;
        mx = fmaxf(mx, x[j]);
    }
    mx = wave_max(mx);
    float se = 0.f;
#pragma unroll
    for (int j = 0; j < MAXV / 64; ++j) se += (j * 64 + lane < Vb) ? __expf(x[j] - mx) : 0.f;
    se = wave_sum(se);
    const float lz = mx + __logf(se);
    float* lp = lps[wave];
#pragma unroll
    for (int j = 0; j < MAXV / 64; ++j) {
        const int v = j * 64 + lane;
        if (v < a.V) {
            const float l = v < Vb ? x[j] - lz : NEG_INF;
            lp[v] = l;
            if (a.log_probs) a.log_probs[((long)t * a.B + b) * a.V + v] = l;
        }
    }
    int Tb = a.input_lens[b];
    Tb = Tb < a.T ? Tb : a.T;
    if (t >= Tb) return;                                          // the recursions never read frames beyond the utterance
    const int L = a.target_lens[b], S = 2 * L + 1;
    float* out = lpe + ((long)b * a.T + t) * a.S_max;
    for (int s = lane; s < a.S_max; s += 64) {
        float l = NEG_INF;
        if (s < S) {
            const int e = (s & 1) ? a.targets[(long)b * a.ldt + (s >> 1)] : a.blank;
            l = (e >= 0 && e < a.V) ? lp[e] : NEG_INF;
        }
        out[s] = l;
    }
}

// ---- 2. the recursions.  grid (B, 1 or 2): y = 0 alpha (+ nll), y = 1 beta.  One wave each; NS states per lane.
template <int NS>
__device__ __forceinline__ void load_row(const float* __restrict__ lpe, long row, int S_max, int lane, float (&dst)[NS]) {
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int s = lane * NS + i;
        dst[i] = s < S_max ? lpe[row * S_max + s] : NEG_INF;
    }
}

template <int NS>
__global__ __launch_bounds__(64) void ctc_recur_kernel(CtcArgs a, const float* __restrict__ lpe, float* __restrict__ beta, int first_dir) {
    const int b = blockIdx.x, lane = threadIdx.x, dir = first_dir + blockIdx.y;
    const int L = a.target_lens[b];
    int Tb = a.input_lens[b];
    Tb = Tb < a.T ? Tb : a.T;
    const int S = 2 * L + 1;
    bool skip[NS];                       // alpha: s-2 -> s allowed; beta: s -> s+2 allowed
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int s = lane * NS + i;
        bool sk = false;
        if (s < S && (s & 1)) {
            const int e = a.targets[(long)b * a.ldt + (s >> 1)];
            if (dir == 0) { if (s >= 3) sk = e != a.targets[(long)b * a.ldt + (s >> 1) - 1]; }
            else { if (s + 2 < S) sk = e != a.targets[(long)b * a.ldt + (s >> 1) + 1]; }
        }
        skip[i] = sk;
    }
    const long base = (long)b * a.T;
    float st[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) st[i] = NEG_INF;
    float* outw = (dir == 0 ? a.alpha : beta) + base * a.S_max;
    // four-deep prefetch ring of lpe rows (static register names: runtime-indexed arrays would go to scratch)
    float r0[NS], r1[NS], r2[NS], r3[NS];
    auto frame = [&](int step) { return dir == 0 ? step : Tb - 1 - step; };
    auto fetch = [&](int step, float (&dst)[NS]) {
        if (step < Tb) load_row<NS>(lpe, base + frame(step), a.S_max, lane, dst);
    };
    fetch(0, r0); fetch(1, r1); fetch(2, r2); fetch(3, r3);
    auto advance = [&](int step, const float (&lp)[NS]) {
        float nw[NS];
        if (step == 0) {
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                const int s = lane * NS + i;
                const bool init = dir == 0 ? (s < 2) : (s == S - 1 || s == S - 2);
                nw[i] = (init && s < S) ? lp[i] : NEG_INF;
            }
        } else if (dir == 0) {
            float p1 = __shfl_up(st[NS - 1], 1, 64), p2 = __shfl_up(st[NS - 2], 1, 64);
            if (lane == 0) { p1 = NEG_INF; p2 = NEG_INF; }
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                const int s = lane * NS + i;
                const float a1 = i >= 1 ? st[i >= 1 ? i - 1 : 0] : p1;
                const float a2 = i >= 2 ? st[i >= 2 ? i - 2 : 0] : (i == 1 ? p1 : p2);
                const float v = lse3(st[i], a1, skip[i] ? a2 : NEG_INF);
                nw[i] = s < S ? v + lp[i] : NEG_INF;
            }
        } else {
            float n1 = __shfl_down(st[0], 1, 64), n2 = __shfl_down(st[1], 1, 64);
            if (lane == 63) { n1 = NEG_INF; n2 = NEG_INF; }
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                const int s = lane * NS + i;
                const float b1 = i + 1 < NS ? st[i + 1 < NS ? i + 1 : 0] : n1;
                const float b2 = i + 2 < NS ? st[i + 2 < NS ? i + 2 : 0] : (i + 2 == NS ? n1 : n2);
                const float v = lse3(st[i], b1, skip[i] ? b2 : NEG_INF);
                nw[i] = s < S ? v + lp[i] : NEG_INF;
            }
        }
        const long t = frame(step);
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            st[i] = nw[i];
            const int s = lane * NS + i;
            if (s < a.S_max) outw[t * a.S_max + s] = nw[i];
        }
    };
    for (int step = 0; step < Tb; step += 4) {
        advance(step, r0);
        fetch(step + 4, r0);
        if (step + 1 < Tb) { advance(step + 1, r1); fetch(step + 5, r1); }
        if (step + 2 < Tb) { advance(step + 2, r2); fetch(step + 6, r2); }
        if (step + 3 < Tb) { advance(step + 3, r3); fetch(step + 7, r3); }
    }
    if (dir != 0) return;
    // log-likelihood = lse(alpha_{T-1}[S-1], alpha_{T-1}[S-2])
    float fin = NEG_INF;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int s = lane * NS + i;
        if (s == S - 1 || s == S - 2) fin = lse2(fin, st[i]);
    }
    const float m = wave_max(fin);
    float ll = NEG_INF;
    if (m != NEG_INF) ll = m + __logf(wave_sum(fin == NEG_INF ? 0.f : __expf(fin - m)));
    if (Tb == 0) ll = (L == 0) ? 0.f : NEG_INF;
    if (lane == 0) a.nll[b] = -ll;
}

__global__ void ctc_reduce_kernel(const float* __restrict__ nll, const int* __restrict__ target_lens, int B, int reduction,
                                  int zero_infinity, float* __restrict__ loss) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (int b = 0; b < B; ++b) {
        float v = nll[b];
        if (zero_infinity && isinf(v)) v = 0.f;
        if (reduction == 1) {
            int tl = target_lens[b];
            tl = tl < 1 ? 1 : tl;
            s += (double)v / tl;
        } else {
            s += (double)v;
        }
    }
    loss[0] = (float)(reduction == 1 ? s / B : s);
}

// ---- 3. gradient rows:  scale_b * (softmax - occupancy).  One wave per row (b, t) of the [B][rows_per_b] output.
// The occupancy of a label is a sum over the states that carry it.  Round 3 scattered exp(.) into LDS with float atomicAdd: the order
// of those additions is not defined, so the last bits of the gradient changed from launch to launch (and Adam's sign-like first steps
// turned that into O(lr) parameter differences: the graph-vs-eager loop test of round 3).  Now ORDER-FIXED: every state's occupancy is
// written to its own LDS word; the blank's sum runs per lane over its (even) states in increasing order and then through the fixed
// shuffle tree; the lane that owns vocabulary entry v adds the states of the labels equal to v in label order.  Same inputs -> same bits.
constexpr int CTC_MAXS = 512;                                     // 2 * 255 + 1 states at most (checked in fill())
template <bool OUT_BF16>
__global__ __launch_bounds__(256) void ctc_grad_kernel(CtcArgs a, const float* __restrict__ lpe, const float* __restrict__ beta,
                                                       const float* __restrict__ grad_out, int reduction, int zero_infinity,
                                                       void* __restrict__ dlogits, long ldd, float extra_scale) {
    __shared__ float ev[4][CTC_MAXS];                             // occupancy of state s
    __shared__ int lab[4][CTC_MAXS / 2];                          // label of odd state 2 i + 1
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long f = (long)blockIdx.x * 4 + wave;
    const bool valid = f < (long)a.B * a.rows_per_b;              // every thread reaches the barrier below
    const int b = valid ? (int)(f / a.rows_per_b) : 0, t = valid ? (int)(f % a.rows_per_b) : 0;
    int Tb = a.input_lens[b];
    Tb = Tb < a.T ? Tb : a.T;
    const int L = a.target_lens[b], S = 2 * L + 1;
    const int Vb = a.vocab_sizes ? a.vocab_sizes[b] : a.V;
    const float nll = a.nll[b];
    float scale = (grad_out ? grad_out[0] : 1.f) * extra_scale;
    if (reduction == 1) scale /= (float)((L < 1 ? 1 : L)) * (float)a.B;
    const bool dead = isinf(nll) || isnan(nll);                  // infeasible alignment: zero_infinity -> zero gradient
    if (dead && zero_infinity) scale = 0.f;
    const bool active = valid && t < Tb && !dead;
    const long r = (long)b * a.rows_per_b + t;
    float blank_part = 0.f;
    if (active) {
        const long off = ((long)b * a.T + t) * a.S_max;
        for (int s = lane; s < S; s += 64) {                     // s and lane have the same parity: even lanes own the blank states
            const float lg = a.alpha[off + s] + beta[off + s] - lpe[off + s] + nll;        // log occupancy, <= 0
            const float o = lg > -80.f ? __expf(lg) : 0.f;
            ev[wave][s] = o;
            if (s & 1) lab[wave][s >> 1] = a.targets[(long)b * a.ldt + (s >> 1)];
            else blank_part += o;
        }
    }
    const float blank_occ = wave_sum(blank_part);                // fixed shuffle tree
    __syncthreads();
    // softmax of the row (recomputed: V <= 256 values)
    const float* row = a.logits + r * a.ldl;
    float x[MAXV / 64];
    float mx = NEG_INF;
#pragma unroll
    for (int j = 0; j < MAXV / 64; ++j) {
        const int v = j * 64 + lane;
        x[j] = (active && v < Vb) ? row[v] : NEG_INF;
        mx = fmaxf(mx, x[j]);
    }
    mx = wave_max(mx);
    float se = 0.f;
#pragma unroll
    for (int j = 0; j < MAXV / 64; ++j) se += (active && j * 64 + lane < Vb) ? __expf(x[j] - mx) : 0.f;
    se = wave_sum(se);
    const float inv = active ? 1.f / se : 0.f;
    if (!valid) return;
#pragma unroll
    for (int j = 0; j < MAXV / 64; ++j) {
        const int v = j * 64 + lane;
        if (j * 64 >= (int)ldd) break;                           // wave-uniform
        float occ = 0.f;
        if (active && j * 64 < a.V) {
            occ = v == a.blank ? blank_occ : 0.f;
            for (int i = 0; i < L; ++i) occ += lab[wave][i] == v ? ev[wave][2 * i + 1] : 0.f;   // LDS broadcasts, label order
        }
        if (v >= (int)ldd) continue;
        float gv = 0.f;
        if (active && v < Vb) gv = scale * (__expf(x[j] - mx) * inv - occ);
        if (OUT_BF16) ((bf16_t*)dlogits)[r * ldd + v] = f2bf(gv);
        else ((float*)dlogits)[r * ldd + v] = gv;
    }
}

// ---- best-path (greedy) CTC decode on the device: frame argmax (first maximum, like torch.argmax) -> collapse repeats -> drop
// blank, over the first T_b = clamp(input_lens[b], 0, T) frames of row b (null: all T); frames at or past T_b are not read.
// sil >= 0 frames the row: the opening silence stands where the label before frame 0 would (`carry`), the closing one follows the
// last round, a frame t is reported as timestep t + 1.  Contract and oracle: include/aptai_hip.h.  One wave per utterance, 64
// frames per round: ballot + prefix popcount compacts the kept labels; every output element is written once, by one lane.
__global__ __launch_bounds__(64) void ctc_greedy_decode_kernel(const float* __restrict__ logits, long ldl, long rows_per_b,
                                                               const int* __restrict__ input_lens, int T, int V, int blank, int sil,
                                                               int* __restrict__ ids_out, int* __restrict__ ts_out, int max_n,
                                                               int* __restrict__ n_out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int Tb = input_lens ? min(max(input_lens[b], 0), T) : T;
    const int framed = sil >= 0 ? 1 : 0;
    auto put = [&](int pos, int id, int ts) {
        if (pos < max_n) ids_out[(long)b * max_n + pos] = id;
        if (pos < max_n && ts_out) ts_out[(long)b * max_n + pos] = ts;
    };
    int count = framed, carry = framed ? sil : -1;               // label of the last frame of the previous round
    if (framed && lane == 0) put(0, sil, 0);
    for (int t0 = 0; t0 < Tb; t0 += 64) {
        const int t = t0 + lane;
        int arg = -1;
        if (t < Tb) {
            const float* row = logits + ((long)b * rows_per_b + t) * ldl;
            float best = row[0];
            arg = 0;
            for (int v = 1; v < V; ++v) {
                const float x = row[v];
                if (x > best) { best = x; arg = v; }
            }
        }
        int prev = __shfl_up(arg, 1, 64);
        if (lane == 0) prev = carry;
        const bool keep = t < Tb && arg != prev && arg != blank;
        const unsigned long long m = __ballot(keep);
        if (keep) put(count + __popcll(m & ((1ull << lane) - 1ull)), arg, t + framed);
        count += __popcll(m);
        carry = __shfl(arg, min(63, Tb - 1 - t0), 64);           // the row's last own frame, in its last round
    }
    if (framed && carry != sil) {                                // wave-uniform
        if (lane == 0) put(count, sil, Tb + 1);
        ++count;
    }
    for (int l = count + lane; l < max_n; l += 64) put(l, 0, 0);
    if (lane == 0) n_out[b] = count;
}

int fill(CtcArgs& a, const char* who, const float* logits, int64_t ldl, int64_t rows_per_b, const int32_t* targets, int64_t ldt,
         const int32_t* input_lens, const int32_t* target_lens, const int32_t* vocab_sizes, int64_t B, int64_t T, int64_t V,
         int blank, float* alpha_ws, float* nll) {
    APTAI_REQUIRE(logits && targets && input_lens && target_lens && alpha_ws && nll, "%s: null pointer", who);
    APTAI_REQUIRE(B > 0 && T > 0 && V > 0 && V <= MAXV && ldl >= V && rows_per_b >= T, "%s: bad sizes (V=%ld, max %d)", who, (long)V, MAXV);
    APTAI_REQUIRE(ldt >= 1 && 2 * ldt + 1 <= 512, "%s: at most 255 labels per utterance (got row length %ld)", who, (long)ldt);
    APTAI_REQUIRE(blank >= 0 && blank < V, "%s: blank out of range", who);
    memset(&a, 0, sizeof(a));
    a.logits = logits; a.ldl = ldl; a.rows_per_b = rows_per_b; a.targets = targets; a.ldt = ldt;
    a.input_lens = input_lens; a.target_lens = target_lens; a.vocab_sizes = vocab_sizes;
    a.B = (int)B; a.T = (int)T; a.V = (int)V; a.blank = blank; a.S_max = (int)(2 * ldt + 1);
    a.alpha = alpha_ws; a.nll = nll;
    return APTAI_OK;
}

}  // namespace

extern "C" int64_t aptai_ctc_workspace_bytes(int64_t B, int64_t T, int64_t ldt) { return 3 * B * T * (2 * ldt + 1) * 4; }

template <int NS>
static void launch_recur(const CtcArgs& a, const float* lpe, float* beta, int first_dir, int ndir, hipStream_t stream) {
    APTAI_LAUNCH(ctc_recur_kernel<NS>, dim3((unsigned)a.B, (unsigned)ndir), dim3(64), 0, stream, a, lpe, beta, first_dir);
}
static void launch_recur_ns(const CtcArgs& a, const float* lpe, float* beta, int first_dir, int ndir, hipStream_t stream) {
    const int ns = (a.S_max + 63) / 64;
    if (ns <= 2) launch_recur<2>(a, lpe, beta, first_dir, ndir, stream);
    else if (ns <= 4) launch_recur<4>(a, lpe, beta, first_dir, ndir, stream);
    else launch_recur<8>(a, lpe, beta, first_dir, ndir, stream);
}

extern "C" int aptai_ctc_fwd(const float* logits, int64_t ldl, int64_t rows_per_b, const int32_t* targets, int64_t ldt,
                             const int32_t* input_lens, const int32_t* target_lens, const int32_t* vocab_sizes, int64_t B,
                             int64_t T, int64_t V, int blank, int reduction, int zero_infinity, float* log_probs_out,
                             float* workspace, float* nll, float* loss, int want_beta, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CtcArgs a;
    int rc = fill(a, "aptai_ctc_fwd", logits, ldl, rows_per_b, targets, ldt, input_lens, target_lens, vocab_sizes, B, T, V, blank,
                  workspace, nll);
    if (rc) return rc;
    APTAI_REQUIRE(loss != nullptr && reduction >= 0 && reduction <= 2, "aptai_ctc_fwd: bad loss/reduction");
    a.log_probs = log_probs_out;
    const long plane = (long)B * T * a.S_max;
    float* beta = workspace + plane;
    float* lpe = workspace + 2 * plane;
    APTAI_LAUNCH(ctc_lpe_kernel, dim3((unsigned)ceil_div(B * T, 4)), dim3(256), 0, stream, a, lpe);
    APTAI_CHECK_LAUNCH("ctc_lpe_kernel");
    launch_recur_ns(a, lpe, beta, 0, want_beta ? 2 : 1, stream);
    APTAI_CHECK_LAUNCH("ctc_recur_kernel");
    if (reduction != 0) {
        APTAI_LAUNCH(ctc_reduce_kernel, dim3(1), dim3(64), 0, stream, (const float*)nll, target_lens, (int)B, reduction,
                     zero_infinity, loss);
        APTAI_CHECK_LAUNCH("ctc_reduce_kernel");
    }
    return APTAI_OK;
}

extern "C" int aptai_ctc_bwd(const float* logits, int64_t ldl, int64_t rows_per_b, const int32_t* targets, int64_t ldt,
                             const int32_t* input_lens, const int32_t* target_lens, const int32_t* vocab_sizes, int64_t B,
                             int64_t T, int64_t V, int blank, int reduction, int zero_infinity, const float* workspace,
                             const float* nll, const float* grad_out, float extra_scale, void* dlogits, int64_t ldd,
                             int out_bf16, int beta_ready, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CtcArgs a;
    int rc = fill(a, "aptai_ctc_bwd", logits, ldl, rows_per_b, targets, ldt, input_lens, target_lens, vocab_sizes, B, T, V, blank,
                  (float*)workspace, (float*)nll);
    if (rc) return rc;
    APTAI_REQUIRE(dlogits != nullptr && ldd >= V && ldd <= MAXV, "aptai_ctc_bwd: bad dlogits (V <= ldd <= %d)", MAXV);
    const long plane = (long)B * T * a.S_max;
    float* beta = (float*)workspace + plane;
    const float* lpe = workspace + 2 * plane;
    if (!beta_ready) {
        launch_recur_ns(a, lpe, beta, 1, 1, stream);
        APTAI_CHECK_LAUNCH("ctc_recur_kernel (beta)");
    }
    const unsigned blocks = (unsigned)ceil_div(B * rows_per_b, 4);
    if (out_bf16) APTAI_LAUNCH((ctc_grad_kernel<true>), dim3(blocks), dim3(256), 0, stream, a, lpe, (const float*)beta, grad_out,
                               reduction, zero_infinity, dlogits, (long)ldd, extra_scale);
    else APTAI_LAUNCH((ctc_grad_kernel<false>), dim3(blocks), dim3(256), 0, stream, a, lpe, (const float*)beta, grad_out, reduction,
                      zero_infinity, dlogits, (long)ldd, extra_scale);
    APTAI_CHECK_LAUNCH("ctc_grad_kernel");
    return APTAI_OK;
}

extern "C" int aptai_ctc_greedy_decode(const float* logits, int64_t ldl, int64_t rows_per_b, const int32_t* input_lens, int64_t B,
                                       int64_t T, int64_t V, int blank, int sil, int32_t* ids_out, int32_t* timesteps_out,
                                       int64_t max_n, int32_t* n_out, void* stream) {
    APTAI_REQUIRE(logits && ids_out && n_out && B > 0 && T > 0 && V > 0 && ldl >= V && rows_per_b >= T && max_n > 0,
                  "aptai_ctc_greedy_decode: bad arguments");
    APTAI_REQUIRE(sil < 0 || (sil < V && sil != blank), "aptai_ctc_greedy_decode: sil (%d) must be below V = %ld and differ from blank (%d)", sil,
                  (long)V, blank);
    APTAI_LAUNCH(ctc_greedy_decode_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, logits, (long)ldl, (long)rows_per_b,
                 input_lens, (int)T, (int)V, blank, sil, ids_out, timesteps_out, (int)max_n, n_out);
    APTAI_CHECK_LAUNCH("ctc_greedy_decode_kernel");
    return APTAI_OK;
}

// ================================================================================================ forced alignment (Viterbi)
// aptai_ctc_viterbi: the best path of a KNOWN transcript through the lattice the recursions above sum over (topology 0), or
// through the blank-free monotonic lattice l1 .. lL (topology 1: the read-out of a forward-sum trained attention).  Three launches:
//   1. vit_gather_kernel (parallel, one wave per frame): xe[b][t][s] = RAW logit of extended state s, lz[b][t] = the frame's
//      log-normaliser.  The path does not depend on lz (the same constant for every state of a frame), so the recursion runs on
//      raw logits: ONE fp32 addition per state and frame, max is exact -> the path is reproducible bit for bit on the host
//      (hostlogic.ctc_forced_align).  lz only enters score / token_score.
//   2. vit_recur_kernel (one wave per utterance): max-plus recursion with the register-resident states, lane shuffles and
//      four-deep row prefetch of ctc_recur_kernel; two-bit backpointers (0 stay, 1 from s-1, 2 from s-2), one word per lane and
//      frame.  The backtrace is a chain of T dependent reads, so it walks LDS: utterances of at most VIT_LDS_BYTES / row bytes
//      frames keep their backpointers in LDS from the start; longer ones write them to the workspace and the backtrace stages
//      them back chunk by chunk with wide coalesced loads - the dependent chain never touches global memory either way.
//   3. vit_spans_kernel (parallel, one workgroup per utterance): spans, score and token_score from frame_token, fixed order.
// Tie rule (include/aptai_hip.h): stay is the incumbent; s-1 replaces it only if strictly greater; then s-2 likewise; the path
// ends in the last state unless the one before it is strictly greater.  No atomics; same inputs -> same bits.
namespace {

constexpr int VIT_LDS_BYTES = 65536;

struct VitArgs {
    const float* logits; long ldl; long rows_per_b;
    const int* targets; long ldt;
    const int* input_lens; const int* target_lens; const int* vocab_sizes;
    int B, T, V, blank, S_max, topology;
};

__device__ __forceinline__ void vit_sizes(const VitArgs& a, int b, int& Tb, int& L, int& S) {
    Tb = a.input_lens[b];
    Tb = Tb < 0 ? 0 : (Tb < a.T ? Tb : a.T);
    L = a.target_lens[b];
    L = L < 0 ? 0 : (L < (int)a.ldt ? L : (int)a.ldt);
    S = a.topology == 0 ? 2 * L + 1 : L;
}

__device__ __forceinline__ int vit_vocab(const VitArgs& a, int b) {
    const int Vb = a.vocab_sizes ? a.vocab_sizes[b] : a.V;
    return Vb < 0 ? 0 : (Vb < a.V ? Vb : a.V);
}

// The log-normaliser of one frame over its first Vb classes, by one wave (every lane returns it).  The narrow and the wide
// alignment both take it from here, so their scores are built from the same bits.
__device__ __forceinline__ float vit_frame_lz(const float* __restrict__ row, int Vb, int lane) {
    float x[MAXV / 64];
    float mx = NEG_INF;
#pragma unroll
    for (int j = 0; j < MAXV / 64; ++j) {
        const int v = j * 64 + lane;
        x[j] = v < Vb ? row[v] : NEG_INF;
        mx = fmaxf(mx, x[j]);
    }
    mx = wave_max(mx);
    float se = 0.f;
#pragma unroll
    for (int j = 0; j < MAXV / 64; ++j) se += (j * 64 + lane < Vb) ? expf(x[j] - mx) : 0.f;
    se = wave_sum(se);
    return mx + logf(se);
}

// ---- 1. raw logit per extended state + log-normaliser per frame.  grid = ceil(B*T/4) blocks of 4 waves, one frame per wave.
__global__ __launch_bounds__(256) void vit_gather_kernel(VitArgs a, float* __restrict__ xe, float* __restrict__ lz) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long f = (long)blockIdx.x * 4 + wave;
    if (f >= (long)a.B * a.T) return;
    const int b = (int)(f / a.T), t = (int)(f % a.T);
    int Tb, L, S;
    vit_sizes(a, b, Tb, L, S);
    if (t >= Tb) return;                                          // the recursion never reads frames beyond the utterance
    const int Vb = vit_vocab(a, b);
    const float* row = a.logits + ((long)b * a.rows_per_b + t) * a.ldl;
    const float z = vit_frame_lz(row, Vb, lane);
    if (lane == 0) lz[f] = z;
    float* out = xe + f * a.S_max;
    for (int s = lane; s < a.S_max; s += 64) {
        float l = NEG_INF;
        if (s < S) {
            const int e = a.topology == 0 ? ((s & 1) ? a.targets[(long)b * a.ldt + (s >> 1)] : a.blank) : a.targets[(long)b * a.ldt + s];
            if (e >= 0 && e < Vb) l = row[e];                    // a label outside the utterance's vocabulary has no path
        }
        out[s] = l;
    }
}

// ---- 2. max-plus recursion + backtrace.  grid B, one wave each; NS states per lane, one backpointer word per lane and frame.
template <int NS> struct VitWord { typedef uint8_t type; };
template <> struct VitWord<8> { typedef uint16_t type; };

template <int NS, int TOPO>
__global__ __launch_bounds__(64) void vit_recur_kernel(VitArgs a, const float* __restrict__ xe, void* __restrict__ bp_ws_,
                                                       int* __restrict__ frame_token) {
    typedef typename VitWord<NS>::type word_t;
    constexpr int CH = VIT_LDS_BYTES / (64 * (int)sizeof(word_t));    // frames per LDS chunk: 1024 (NS <= 4) or 512 (NS = 8)
    constexpr int SH = NS == 2 ? 1 : (NS == 4 ? 2 : 3);
    __shared__ __attribute__((aligned(16))) word_t bpl[CH * 64];
    const int b = blockIdx.x, lane = threadIdx.x;
    int Tb, L, S;
    vit_sizes(a, b, Tb, L, S);
    int* ft = frame_token + (long)b * a.T;
    const bool in_lds = Tb <= CH;                                 // wave-uniform
    word_t* bp_ws = (word_t*)bp_ws_ + (long)b * a.T * 64;
    bool skip[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int s = lane * NS + i;
        bool sk = false;
        if (TOPO == 0 && s < S && (s & 1) && s >= 3)
            sk = a.targets[(long)b * a.ldt + (s >> 1)] != a.targets[(long)b * a.ldt + (s >> 1) - 1];
        skip[i] = sk;
    }
    const long base = (long)b * a.T;
    float st[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) st[i] = NEG_INF;
    float r0[NS], r1[NS], r2[NS], r3[NS];                         // four-deep prefetch ring, static names (see ctc_recur_kernel)
    auto fetch = [&](int step, float (&dst)[NS]) {
        if (step < Tb) load_row<NS>(xe, base + step, a.S_max, lane, dst);
    };
    fetch(0, r0); fetch(1, r1); fetch(2, r2); fetch(3, r3);
    auto advance = [&](int step, const float (&x)[NS]) {
        float nw[NS];
        unsigned word = 0;
        if (step == 0) {
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                const int s = lane * NS + i;
                const bool init = TOPO == 0 ? (s < 2) : (s == 0);
                nw[i] = (init && s < S) ? x[i] : NEG_INF;
            }
        } else {
            float p1 = __shfl_up(st[NS - 1], 1, 64), p2 = __shfl_up(st[NS - 2], 1, 64);
            if (lane == 0) { p1 = NEG_INF; p2 = NEG_INF; }
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                const int s = lane * NS + i;
                const float a1 = i >= 1 ? st[i >= 1 ? i - 1 : 0] : p1;
                const float a2 = i >= 2 ? st[i >= 2 ? i - 2 : 0] : (i == 1 ? p1 : p2);
                float best = st[i];
                unsigned c = 0;
                if (a1 > best) { best = a1; c = 1; }
                if (TOPO == 0 && skip[i] && a2 > best) { best = a2; c = 2; }
                nw[i] = s < S ? best + x[i] : NEG_INF;           // the ONE fp32 addition per state and frame
                word |= c << (2 * i);
            }
        }
#pragma unroll
        for (int i = 0; i < NS; ++i) st[i] = nw[i];
        if (in_lds) bpl[step * 64 + lane] = (word_t)word;
        else bp_ws[(long)step * 64 + lane] = (word_t)word;
    };
    for (int step = 0; step < Tb; step += 4) {
        advance(step, r0);
        fetch(step + 4, r0);
        if (step + 1 < Tb) { advance(step + 1, r1); fetch(step + 5, r1); }
        if (step + 2 < Tb) { advance(step + 2, r2); fetch(step + 6, r2); }
        if (step + 3 < Tb) { advance(step + 3, r3); fetch(step + 7, r3); }
    }
    // final state: the last one unless the one before it is strictly greater
    float vlast = NEG_INF, vprev = NEG_INF;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int s = lane * NS + i;
        if (s == S - 1) vlast = st[i];
        if (TOPO == 0 && s == S - 2) vprev = st[i];
    }
    vlast = wave_max(vlast);                                      // one lane holds the value, the others -inf: exact
    vprev = wave_max(vprev);
    int s = S - 1;
    float best = vlast;
    if (vprev > vlast) { s = S - 2; best = vprev; }
    const bool feasible = Tb > 0 && S > 0 && best > NEG_INF;
    for (int t = (feasible ? Tb : 0) + lane; t < a.T; t += 64) ft[t] = -2;
    if (!feasible) return;                                        // wave-uniform
    if (!in_lds) __threadfence();                                 // this wave's backpointer stores before its own loads below
    __syncthreads();
    int mine = -2;
    for (int c0 = ((Tb - 1) / CH) * CH; c0 >= 0; c0 -= CH) {
        const int c1 = Tb < c0 + CH ? Tb : c0 + CH;
        if (!in_lds) {
            const uint4* src = (const uint4*)(bp_ws + (long)c0 * 64);
            uint4* dst = (uint4*)bpl;
            const int n16 = (c1 - c0) * 64 * (int)sizeof(word_t) / 16;
            for (int i = lane; i < n16; i += 64) dst[i] = src[i];
            __syncthreads();
        }
        for (int t = c1 - 1; t >= c0; --t) {
            const int tok = TOPO == 0 ? ((s & 1) ? (s >> 1) : -1) : s;
            if (lane == (t & 63)) mine = tok;
            if ((t & 63) == 0 && t + lane < Tb) ft[t + lane] = mine;
            if (t > 0) {
                const unsigned w = bpl[(t - c0) * 64 + (s >> SH)];
                s -= (int)((w >> (2 * (s & (NS - 1)))) & 3u);
                s = __builtin_amdgcn_readfirstlane(s < 0 ? 0 : s);
            }
        }
        __syncthreads();
    }
}

// ---- 3. spans, score, token_score from frame_token.  grid B, 256 threads; every sum in a fixed order.
__global__ __launch_bounds__(256) void vit_spans_kernel(VitArgs a, const float* __restrict__ xe, const float* __restrict__ lz,
                                                        const int* __restrict__ frame_token, int* __restrict__ spans,
                                                        float* __restrict__ score, float* __restrict__ token_score) {
    __shared__ int sp[256][2];
    __shared__ float red[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    int Tb, L, S;
    vit_sizes(a, b, Tb, L, S);
    const int* ft = frame_token + (long)b * a.T;
    const long base = (long)b * a.T;
    sp[tid][0] = -1;
    sp[tid][1] = -1;
    __syncthreads();
    const bool feasible = Tb > 0 ? ft[0] != -2 : L == 0;
    float part = 0.f;
    if (feasible) {
        for (int t = tid; t < Tb; t += 256) {
            const int k = ft[t];
            const int state = a.topology == 0 ? (k < 0 ? 0 : 2 * k + 1) : k;     // every blank state carries the same logit
            part += xe[(base + t) * a.S_max + state] - lz[base + t];
            if (k >= 0) {
                if (t == 0 || ft[t - 1] != k) sp[k][0] = t;
                if (t == Tb - 1 || ft[t + 1] != k) sp[k][1] = t + 1;
            }
        }
    }
    red[tid] = part;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) score[b] = feasible ? red[0] : NEG_INF;
    if (tid < (int)a.ldt) {
        const int f0 = sp[tid][0], f1 = sp[tid][1];
        spans[((long)b * a.ldt + tid) * 2] = f0;
        spans[((long)b * a.ldt + tid) * 2 + 1] = f1;
        if (token_score) {
            float v = NEG_INF;
            if (f0 >= 0) {
                const int state = a.topology == 0 ? 2 * tid + 1 : tid;
                float acc = 0.f;
                for (int t = f0; t < f1; ++t) acc += xe[(base + t) * a.S_max + state] - lz[base + t];
                v = acc / (float)(f1 - f0);
            }
            token_score[(long)b * a.ldt + tid] = v;
        }
    }
}

// workspace: xe [B*T][S_max] fp32 | lz [B*T] fp32 | backpointers [B*T][64] words of at most 2 bytes; every part 16-byte aligned
struct VitLayout { int64_t xe, lz, bp, total; };
VitLayout vit_layout(int64_t B, int64_t T, int64_t ldt) {
    VitLayout l;
    const int64_t S_max = 2 * ldt + 1;
    l.xe = 0;
    l.lz = (B * T * S_max * 4 + 15) / 16 * 16;
    l.bp = l.lz + (B * T * 4 + 15) / 16 * 16;
    l.total = l.bp + B * T * 64 * 2;
    return l;
}

template <int NS>
void launch_vit(const VitArgs& a, const float* xe, void* bp, int32_t* frame_token, hipStream_t stream) {
    if (a.topology == 0) APTAI_LAUNCH((vit_recur_kernel<NS, 0>), dim3((unsigned)a.B), dim3(64), 0, stream, a, xe, bp, frame_token);
    else APTAI_LAUNCH((vit_recur_kernel<NS, 1>), dim3((unsigned)a.B), dim3(64), 0, stream, a, xe, bp, frame_token);
}

}  // namespace

extern "C" int64_t aptai_ctc_viterbi_workspace_bytes(int64_t B, int64_t T, int64_t ldt) { return vit_layout(B, T, ldt).total; }

extern "C" int aptai_ctc_viterbi(const float* logits, int64_t ldl, int64_t rows_per_b, const int32_t* targets, int64_t ldt,
                                 const int32_t* input_lens, const int32_t* target_lens, const int32_t* vocab_sizes, int64_t B,
                                 int64_t T, int64_t V, int blank, int topology, void* workspace, int32_t* frame_token,
                                 int32_t* spans, float* score, float* token_score, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char* who = "aptai_ctc_viterbi";
    APTAI_REQUIRE(logits && targets && input_lens && target_lens && workspace && frame_token && spans && score, "%s: null pointer", who);
    APTAI_REQUIRE(B > 0 && T > 0 && V > 0 && V <= MAXV && ldl >= V && rows_per_b >= T, "%s: bad sizes (V=%ld, max %d)", who, (long)V, MAXV);
    APTAI_REQUIRE(ldt >= 1 && 2 * ldt + 1 <= 512, "%s: at most 255 labels per utterance (got row length %ld)", who, (long)ldt);
    APTAI_REQUIRE(topology == 0 || topology == 1, "%s: topology must be 0 (CTC) or 1 (monotonic, no blank)", who);
    APTAI_REQUIRE(topology == 1 || (blank >= 0 && blank < V), "%s: blank out of range", who);
    APTAI_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: workspace must be 16-byte aligned", who);
    VitArgs a;
    memset(&a, 0, sizeof(a));
    a.logits = logits; a.ldl = ldl; a.rows_per_b = rows_per_b; a.targets = targets; a.ldt = ldt;
    a.input_lens = input_lens; a.target_lens = target_lens; a.vocab_sizes = vocab_sizes;
    a.B = (int)B; a.T = (int)T; a.V = (int)V; a.blank = blank; a.topology = topology;
    a.S_max = (int)(topology == 0 ? 2 * ldt + 1 : ldt);
    const VitLayout l = vit_layout(B, T, ldt);
    float* xe = (float*)((char*)workspace + l.xe);
    float* lz = (float*)((char*)workspace + l.lz);
    void* bp = (char*)workspace + l.bp;
    APTAI_LAUNCH(vit_gather_kernel, dim3((unsigned)ceil_div(B * T, 4)), dim3(256), 0, stream, a, xe, lz);
    APTAI_CHECK_LAUNCH("vit_gather_kernel");
    const int ns = (a.S_max + 63) / 64;
    if (ns <= 2) launch_vit<2>(a, xe, bp, frame_token, stream);
    else if (ns <= 4) launch_vit<4>(a, xe, bp, frame_token, stream);
    else launch_vit<8>(a, xe, bp, frame_token, stream);
    APTAI_CHECK_LAUNCH("vit_recur_kernel");
    APTAI_LAUNCH(vit_spans_kernel, dim3((unsigned)B), dim3(256), 0, stream, a, (const float*)xe, (const float*)lz,
                 (const int*)frame_token, spans, score, token_score);
    APTAI_CHECK_LAUNCH("vit_spans_kernel");
    return APTAI_OK;
}

// ================================================================================================ forced alignment, wide lattice
// aptai_ctc_viterbi_wide: the contract of aptai_ctc_viterbi with topology 0 for transcripts of up to
// APTAI_CTC_VITERBI_WIDE_MAX_LABELS labels (a long recording against its whole transcript).  Three launches:
//   1. vitw_lz_kernel (parallel, one wave per frame): lz[b][t] through vit_frame_lz, the narrow kernel's own reduction.  There is
//      no per-state emission matrix: every state fetches its raw logit from the frame's row.
//   2. vitw_recur_kernel (one workgroup per recording, up to 16 waves): NS consecutive states per thread in registers, the labels
//      of its odd states beside them; the even states all read the one blank logit.  Neighbours: lane to lane by shuffle, wave to
//      wave through a double-buffered LDS pair per wave, so ONE barrier per frame orders everything.  The logits rows are staged
//      into an LDS ring by wave 0, four frames at a time and four frames ahead, with the next four in flight in registers.
//      Backpointers: two bits per state, packed from state 0 upwards into rows of ceil(S_max / 16) words, written coalesced, four
//      frames at a time.  The backtrace never
//      reads global memory in its chain: a path moves at most two states per frame, so a chunk of VITW_CHUNK frames ending in
//      state s can only visit states [s - 2 (VITW_CHUNK - 1), s], at most VITW_BAND words per frame; the whole group stages that
//      band into LDS, then one wave walks it and writes frame_token in 64-frame pieces.
//   3. vitw_spans_kernel (parallel, one workgroup per recording): spans from the frames where frame_token changes, score and
//      token_score in the summation orders of vit_spans_kernel, so that for ldt <= 255 all four outputs equal the narrow kernel's.
// Tie rule: as above.  No atomics; same inputs -> same bits; 64-bit offsets wherever B, T and the row width multiply.
namespace {

constexpr int VITW_CHUNK = 256;                                   // frames per backtrace chunk
constexpr int VITW_BAND = 33;                                     // 2 (VITW_CHUNK - 1) + 1 = 511 states touch at most 33 words of 16
constexpr int VITW_RING = 8;                                      // staged logits rows: the turn being read and the next
constexpr int VITW_ROW = MAXV + 1;                                // [MAXV] holds -inf: where a label outside [0, MAXV) points
constexpr int VITW_MAX_THREADS = 1024;

// ---- 1. log-normaliser per frame.  grid = ceil(B*T/4) blocks of 4 waves, one frame per wave.
__global__ __launch_bounds__(256) void vitw_lz_kernel(VitArgs a, float* __restrict__ lz) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long f = (long)blockIdx.x * 4 + wave;
    if (f >= (long)a.B * a.T) return;
    const int b = (int)(f / a.T), t = (int)(f % a.T);
    int Tb, L, S;
    vit_sizes(a, b, Tb, L, S);
    if (t >= Tb) return;
    const float z = vit_frame_lz(a.logits + ((long)b * a.rows_per_b + t) * a.ldl, vit_vocab(a, b), lane);
    if (lane == 0) lz[f] = z;
}

// this wave's LDS traffic done, then the group's barrier: vector loads and stores stay in flight across it
__device__ __forceinline__ void vitw_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Rows f0 .. f0 + 3 of the logits, columns j * 64 + lane for j < NJ, into registers: unconditional loads from clamped addresses
// (a frame at or beyond Tb repeats the last one and is never read; a class at or beyond Vb becomes -inf when staged), so that
// nothing branches around a load or waits for it here.  Needs Tb >= 1.
template <int NJ>
__device__ __forceinline__ void vitw_fetch4(const float* __restrict__ logits, long ldl, int f0, int Tb, int Vb, int lane,
                                            float (&q)[4][MAXV / 64]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long f = f0 + k < Tb ? f0 + k : Tb - 1;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int v = j * 64 + lane;
            q[k][j] = logits[f * ldl + (v < Vb ? v : 0)];          // masked when staged: nothing here touches the loaded value
        }
    }
}
template <int NJ>
__device__ __forceinline__ void vitw_stage4(float (&rows)[VITW_RING][VITW_ROW], int f0, int Vb, int lane, const float (&q)[4][MAXV / 64]) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < NJ; ++j) rows[(f0 + k) & (VITW_RING - 1)][j * 64 + lane] = j * 64 + lane < Vb ? q[k][j] : NEG_INF;
}

// ---- 2. max-plus recursion + backtrace.  grid B, blockDim.x = 64 * ceil(S_max / (64 NS)) threads.
// NJ = ceil(V / 64) columns per lane of a staged row, 1 or 4: a template parameter so that the staged values have one home in the
// registers (a runtime choice made the compiler copy them at the join, and wait for the loads it had just issued).
template <int NS, int NJ>
__global__ __launch_bounds__(VITW_MAX_THREADS) void vitw_recur_kernel(VitArgs a, uint32_t* __restrict__ bp_ws, int* __restrict__ frame_token) {
    constexpr int NL = NS / 2;                                    // labels (odd states) per thread
    __shared__ float rows[VITW_RING][VITW_ROW];
    __shared__ float edge[2][VITW_MAX_THREADS / 64][2];           // [frame parity][wave]{last state, the one before it}
    __shared__ uint32_t band[VITW_CHUNK * VITW_BAND];
    __shared__ float fin[2];
    __shared__ int s_next;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x;
    int Tb, L, S;
    vit_sizes(a, b, Tb, L, S);
    const int Vb = vit_vocab(a, b);
    const long W = (a.S_max + 15) >> 4;                           // backpointer words per frame
    uint32_t* bp = bp_ws + (long)b * a.T * W;
    int* ft = frame_token + (long)b * a.T;
    const float* logits = a.logits + (long)b * a.rows_per_b * a.ldl;
    const int* tg = a.targets + (long)b * a.ldt;
    const int s0 = tid * NS;                                      // even: state s0 + i is blank for even i, label (s0 + i) >> 1 for odd i
    const int nvalid = S - s0;                                    // states i < nvalid exist
    int lab[NL];
    unsigned skip = 0;                                            // bit j: state s0 + 2j + 1 may come from two states below
#pragma unroll
    for (int j = 0; j < NL; ++j) {
        const int k = (s0 >> 1) + j;
        const int kc = k < L ? k : 0;                             // loads from clamped positions: no branch around them (L == 0: slot 0, unused)
        const int tk = tg[kc], tp = tg[kc > 0 ? kc - 1 : 0];
        lab[j] = (k < L && tk >= 0 && tk < MAXV) ? tk : MAXV;     // classes at or beyond Vb hold -inf in the staged row
        if (k < L && k >= 1 && tk != tp) skip |= 1u << j;
    }
    for (int i = tid; i < VITW_RING * VITW_ROW; i += nthreads) (&rows[0][0])[i] = NEG_INF;
    if (tid < 2) fin[tid] = NEG_INF;
    __syncthreads();
    // Wave 0 stages the logits rows, four frames (one turn of the loop below) at a time.  At the head of a turn it writes the rows it
    // requested a turn ago into the half of the ring that no frame of this turn reads and requests the next four; right behind
    // that every wave stores the backpointer words of the turn before.  The vector-memory counter counts loads and stores
    // together, so the compiler's wait in front of the staged values is a wait for everything: placed here, it finds loads and
    // stores that have had a whole turn to complete, and no frame inside the turn waits for memory.
    float q[4][MAXV / 64];
    if (wave == 0 && Tb > 0) {
        vitw_fetch4<NJ>(logits, a.ldl, 0, Tb, Vb, lane, q);
        vitw_stage4<NJ>(rows, 0, Vb, lane, q);
        vitw_fetch4<NJ>(logits, a.ldl, 4, Tb, Vb, lane, q);
    }
    __syncthreads();
    float st[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) st[i] = NEG_INF;
    // two bits per state from state 0 upwards: thread tid owns bits [2 NS tid, 2 NS (tid + 1)) of the frame's row
    auto store_word = [&](int t, unsigned word) {
        uint32_t* bpr = bp + (long)t * W;
        if (s0 < a.S_max) {
            if (NS == 16) bpr[tid] = word;
            else if (NS == 8) ((uint16_t*)bpr)[tid] = (uint16_t)word;
            else if (NS == 4) ((uint8_t*)bpr)[tid] = (uint8_t)word;
            else if (!(tid & 1)) ((uint8_t*)bpr)[tid >> 1] = (uint8_t)word;      // NS == 2: the even thread holds the pair's byte
        }
    };
    // one frame: reads rows[t & 7] and edge[(t - 1) & 1], writes edge[t & 1]; the barrier at its end makes that visible, and what the
    // next frame overwrites (edge[(t + 1) & 1]) was last read before that barrier.  LDS only: loads and stores stay in flight.
    auto advance = [&](int t, unsigned& kept) {
        const float* row = rows[t & (VITW_RING - 1)];
        const float xb = row[a.blank];
        float xl[NL];
#pragma unroll
        for (int j = 0; j < NL; ++j) xl[j] = row[lab[j]];
        float nw[NS];
        unsigned word = 0;
        if (t == 0) {
#pragma unroll
            for (int i = 0; i < NS; ++i) nw[i] = (s0 + i < 2 && i < nvalid) ? ((i & 1) ? xl[i >> 1] : xb) : NEG_INF;
        } else {
            const int pw = wave > 0 ? wave - 1 : 0;
            const float e1 = edge[(t - 1) & 1][pw][0], e2 = edge[(t - 1) & 1][pw][1];
            float p1 = __shfl_up(st[NS - 1], 1, 64), p2 = __shfl_up(st[NS - 2], 1, 64);
            if (lane == 0) { p1 = wave > 0 ? e1 : NEG_INF; p2 = wave > 0 ? e2 : NEG_INF; }
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                const float a1 = i >= 1 ? st[i >= 1 ? i - 1 : 0] : p1;
                const float a2 = i >= 2 ? st[i >= 2 ? i - 2 : 0] : (i == 1 ? p1 : p2);
                float best = st[i];
                unsigned c = 0;
                if (a1 > best) { best = a1; c = 1; }
                if ((i & 1) && ((skip >> (i >> 1)) & 1u) && a2 > best) { best = a2; c = 2; }
                nw[i] = i < nvalid ? best + ((i & 1) ? xl[i >> 1] : xb) : NEG_INF;   // the ONE fp32 addition per state and frame
                word |= c << (2 * i);
            }
        }
#pragma unroll
        for (int i = 0; i < NS; ++i) st[i] = nw[i];
        if (lane == 63) { edge[t & 1][wave][0] = nw[NS - 1]; edge[t & 1][wave][1] = nw[NS - 2]; }
        kept = NS == 2 ? (word | (__shfl_down(word, 1, 64) << 4)) : word;
        vitw_lds_barrier();
    };
    unsigned w0 = 0, w1 = 0, w2 = 0, w3 = 0;
    for (int t = 0; t < Tb; t += 4) {                             // Tb is uniform over the group: every barrier is reached by all
        if (wave == 0) {                                          // rows t + 4 .. t + 7 replace those of the turn before in the ring
            vitw_stage4<NJ>(rows, t + 4, Vb, lane, q);
            vitw_fetch4<NJ>(logits, a.ldl, t + 8, Tb, Vb, lane, q);
        }
        if (t > 0) { store_word(t - 4, w0); store_word(t - 3, w1); store_word(t - 2, w2); store_word(t - 1, w3); }
        advance(t, w0);
        if (t + 1 < Tb) advance(t + 1, w1);
        if (t + 2 < Tb) advance(t + 2, w2);
        if (t + 3 < Tb) advance(t + 3, w3);
    }
    if (Tb > 0) {
        const int t = ((Tb - 1) >> 2) << 2;                       // the last turn's words
        store_word(t, w0);
        if (t + 1 < Tb) store_word(t + 1, w1);
        if (t + 2 < Tb) store_word(t + 2, w2);
        if (t + 3 < Tb) store_word(t + 3, w3);
    }
    // final state: the last one unless the one before it is strictly greater
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        if (s0 + i == S - 1) fin[0] = st[i];
        if (s0 + i == S - 2) fin[1] = st[i];
    }
    __syncthreads();
    int s = S - 1;
    float best = fin[0];
    if (fin[1] > best) { s = S - 2; best = fin[1]; }
    const bool feasible = Tb > 0 && best > NEG_INF;
    for (int t = (feasible ? Tb : 0) + tid; t < a.T; t += nthreads) ft[t] = -2;
    if (!feasible) return;                                        // uniform over the group
    __threadfence();                                              // the group's backpointer stores before its own loads below
    __syncthreads();
    int mine = -2;
    for (int c0 = ((Tb - 1) / VITW_CHUNK) * VITW_CHUNK; c0 >= 0; c0 -= VITW_CHUNK) {
        const int c1 = Tb < c0 + VITW_CHUNK ? Tb : c0 + VITW_CHUNK, n = c1 - c0;
        const int low = s - 2 * (n - 1);
        const int wlo = (low < 0 ? 0 : low) >> 4, bw = (s >> 4) - wlo + 1;        // bw <= VITW_BAND
        for (int i = tid; i < n * bw; i += nthreads) {
            const int r = i / bw, c = i - r * bw;
            band[r * VITW_BAND + c] = bp[(long)(c0 + r) * W + wlo + c];
        }
        __syncthreads();
        if (wave == 0) {
            for (int t = c1 - 1; t >= c0; --t) {
                const int tok = (s & 1) ? (s >> 1) : -1;
                if (lane == (t & 63)) mine = tok;
                if ((t & 63) == 0 && t + lane < Tb) ft[t + lane] = mine;
                if (t > 0) {
                    const unsigned w = band[(t - c0) * VITW_BAND + (s >> 4) - wlo];
                    s -= (int)((w >> (2 * (s & 15))) & 3u);
                    s = __builtin_amdgcn_readfirstlane(s < 0 ? 0 : s);
                }
            }
            if (lane == 0) s_next = s;
        }
        __syncthreads();
        s = s_next;
    }
}

// ---- 3. spans, score, token_score from frame_token, for any ldt.  grid B, 256 threads; the orders of vit_spans_kernel.
__global__ __launch_bounds__(256) void vitw_spans_kernel(VitArgs a, const float* __restrict__ lz, const int* __restrict__ frame_token,
                                                         int* spans, float* __restrict__ score, float* __restrict__ token_score) {
    __shared__ float red[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    int Tb, L, S;
    vit_sizes(a, b, Tb, L, S);
    const int Vb = vit_vocab(a, b);
    const int* ft = frame_token + (long)b * a.T;
    const int* tg = a.targets + (long)b * a.ldt;
    int* sp = spans + (long)b * a.ldt * 2;
    const float* logits = a.logits + (long)b * a.rows_per_b * a.ldl;
    const long base = (long)b * a.T;
    auto logp = [&](int t, int e) {                               // a frame of a feasible path only meets classes with a logit
        const float x = (e >= 0 && e < Vb) ? logits[(long)t * a.ldl + e] : NEG_INF;
        return x - lz[base + t];
    };
    for (long i = tid; i < 2 * a.ldt; i += 256) sp[i] = -1;
    __syncthreads();
    const bool feasible = Tb > 0 ? ft[0] != -2 : L == 0;
    float part = 0.f;
    if (feasible) {
        for (int t = tid; t < Tb; t += 256) {
            const int k = ft[t];
            part += logp(t, k < 0 ? a.blank : tg[k]);
            if (k >= 0) {
                if (t == 0 || ft[t - 1] != k) sp[2 * k] = t;
                if (t == Tb - 1 || ft[t + 1] != k) sp[2 * k + 1] = t + 1;
            }
        }
    }
    red[tid] = part;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) score[b] = feasible ? red[0] : NEG_INF;
    if (!token_score) return;
    for (int k = tid; k < (int)a.ldt; k += 256) {
        const int f0 = sp[2 * k], f1 = sp[2 * k + 1];
        float v = NEG_INF;
        if (f0 >= 0) {
            const int e = tg[k];
            float acc = 0.f;
            for (int t = f0; t < f1; ++t) acc += logp(t, e);
            v = acc / (float)(f1 - f0);
        }
        token_score[(long)b * a.ldt + k] = v;
    }
}

// workspace: lz [B*T] fp32 | backpointers [B][T][ceil(S_max / 16)] words; both parts 16-byte aligned
struct VitwLayout { int64_t lz, bp, total; };
VitwLayout vitw_layout(int64_t B, int64_t T, int64_t ldt) {
    VitwLayout l;
    l.lz = 0;
    l.bp = (B * T * 4 + 15) / 16 * 16;
    l.total = l.bp + B * T * ((2 * ldt + 1 + 15) / 16) * 4;
    return l;
}

template <int NS>
void launch_vitw(const VitArgs& a, uint32_t* bp, int32_t* frame_token, hipStream_t stream) {
    const int threads = (int)ceil_div(ceil_div(a.S_max, NS), 64) * 64;
    if (a.V <= 64) APTAI_LAUNCH((vitw_recur_kernel<NS, 1>), dim3((unsigned)a.B), dim3((unsigned)threads), 0, stream, a, bp, frame_token);
    else APTAI_LAUNCH((vitw_recur_kernel<NS, 4>), dim3((unsigned)a.B), dim3((unsigned)threads), 0, stream, a, bp, frame_token);
}

}  // namespace

extern "C" int64_t aptai_ctc_viterbi_wide_workspace_bytes(int64_t B, int64_t T, int64_t ldt) { return vitw_layout(B, T, ldt).total; }

extern "C" int aptai_ctc_viterbi_wide(const float* logits, int64_t ldl, int64_t rows_per_b, const int32_t* targets, int64_t ldt,
                                      const int32_t* input_lens, const int32_t* target_lens, const int32_t* vocab_sizes, int64_t B,
                                      int64_t T, int64_t V, int blank, int topology, void* workspace, int32_t* frame_token,
                                      int32_t* spans, float* score, float* token_score, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char* who = "aptai_ctc_viterbi_wide";
    APTAI_REQUIRE(logits && targets && input_lens && target_lens && workspace && frame_token && spans && score, "%s: null pointer", who);
    APTAI_REQUIRE(topology == 0, "%s: only topology 0 (CTC) has a wide lattice; topology %d goes through aptai_ctc_viterbi", who, topology);
    APTAI_REQUIRE(B > 0 && T > 0 && B <= INT32_MAX / T && V > 0 && V <= MAXV && ldl >= V && rows_per_b >= T,
                  "%s: bad sizes (B*T=%ld*%ld must stay below 2^31, V=%ld, max %d)", who, (long)B, (long)T, (long)V, MAXV);
    APTAI_REQUIRE(ldt >= 1 && ldt <= APTAI_CTC_VITERBI_WIDE_MAX_LABELS, "%s: at most %d labels per recording (got row length %ld)", who,
                  APTAI_CTC_VITERBI_WIDE_MAX_LABELS, (long)ldt);
    APTAI_REQUIRE(blank >= 0 && blank < V, "%s: blank out of range", who);
    APTAI_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: workspace must be 16-byte aligned", who);
    VitArgs a;
    memset(&a, 0, sizeof(a));
    a.logits = logits; a.ldl = ldl; a.rows_per_b = rows_per_b; a.targets = targets; a.ldt = ldt;
    a.input_lens = input_lens; a.target_lens = target_lens; a.vocab_sizes = vocab_sizes;
    a.B = (int)B; a.T = (int)T; a.V = (int)V; a.blank = blank; a.topology = 0;
    a.S_max = (int)(2 * ldt + 1);
    const VitwLayout l = vitw_layout(B, T, ldt);
    float* lz = (float*)((char*)workspace + l.lz);
    uint32_t* bp = (uint32_t*)((char*)workspace + l.bp);
    APTAI_LAUNCH(vitw_lz_kernel, dim3((unsigned)ceil_div(B * T, 4)), dim3(256), 0, stream, a, lz);
    APTAI_CHECK_LAUNCH("vitw_lz_kernel");
    // eight waves where 16 states per thread allow it: NS = the fewest states per thread that keep the group at 512 threads
    if (a.S_max <= 512 * 2) launch_vitw<2>(a, bp, frame_token, stream);
    else if (a.S_max <= 512 * 4) launch_vitw<4>(a, bp, frame_token, stream);
    else if (a.S_max <= 512 * 8) launch_vitw<8>(a, bp, frame_token, stream);
    else launch_vitw<16>(a, bp, frame_token, stream);
    APTAI_CHECK_LAUNCH("vitw_recur_kernel");
    APTAI_LAUNCH(vitw_spans_kernel, dim3((unsigned)B), dim3(256), 0, stream, a, (const float*)lz, (const int*)frame_token, spans, score,
                 token_score);
    APTAI_CHECK_LAUNCH("vitw_spans_kernel");
    return APTAI_OK;
}
