// Multi-tensor Adam (torch.optim.Adam semantics: train/train_aptai.py:350-356 - betas, eps OUTSIDE the square root divided by
// sqrt(bias_correction2), L2 weight decay added to the gradient, no amsgrad) over a device job table, one launch per
// parameter group.  HBM-bound: 16 B read + 12 B written per parameter, plus the optional refreshed compute copy
// (bf16 for GEMM weights, fp32 for packed biases), which replaces a separate cast pass over the parameters.
#include "common.h"

namespace {

struct AdamArgs {
    const int64_t* table;       // static rows of 6: {param, exp_avg, exp_avg_sq, copy_dst (0 = none), n, copy_kind (0 bf16 / 1 fp32)}
    const int64_t* dyn;         // per-step rows of 2: {grad (0 = no gradient this step: skip), step count of THIS update (>= 1)}
    float lr, beta1, beta2, eps, weight_decay;
    float bc1, bc2_sqrt;        // filled per block from the job's own step count
};

constexpr int ADAM_CHUNK = 4096;    // elements per block: 256 threads x 4 x 4

__device__ __forceinline__ float adam_one(float p, float g, float& m, float& v, const AdamArgs& a) {
    g = fmaf(a.weight_decay, p, g);
    m = fmaf(a.beta1, m, (1.0f - a.beta1) * g);
    v = fmaf(a.beta2, v, (1.0f - a.beta2) * g * g);
    const float denom = __fsqrt_rn(v) / a.bc2_sqrt + a.eps;
    return p - (a.lr / a.bc1) * (m / denom);
}

// SCALED = false is the plain step.  SCALED = true multiplies every gradient by *scale first (the global-norm clip coefficient
// grad_norm_final_kernel left on the device: one scalar load per block, one rounded fp32 multiply per element), then runs the
// same adam_one - so weight decay is added to the SCALED gradient, as torch.nn.utils.clip_grad_norm_ + torch.optim.Adam do.
template <bool SCALED>
__global__ __launch_bounds__(256) void adam_multi_kernel(AdamArgs a, const float* __restrict__ scale) {
    const int64_t* job = a.table + (long)blockIdx.y * 6;
    const int64_t* dyn = a.dyn + (long)blockIdx.y * 2;
    const long n = job[4];
    const long base = (long)blockIdx.x * ADAM_CHUNK;
    const float* g = (const float*)dyn[0];
    if (base >= n || g == nullptr) return;
    float coef = 1.0f;
    if (SCALED) coef = *scale;
    // bias corrections of this parameter's own step count (parameters skipped by LayerDrop lag behind), in double like
    // the Python reference; every thread computes the same two values
    // (one lane per block evaluates the two double-precision powers - 256 threads each did, ~200 instructions beside 16 elements of work)
    __shared__ float bc[2];
    if (threadIdx.x == 0) {
        const double step = (double)dyn[1];
        bc[0] = (float)(1.0 - pow((double)a.beta1, step));
        bc[1] = (float)sqrt(1.0 - pow((double)a.beta2, step));
    }
    __syncthreads();
    a.bc1 = bc[0];
    a.bc2_sqrt = bc[1];
    float* p = (float*)job[0];
    float* m = (float*)job[1];
    float* v = (float*)job[2];
    void* copy = (void*)job[3];
    const bool copy_f32 = job[5] != 0;
    const bool vec = (n % 4 == 0) && ((job[0] | job[1] | job[2] | dyn[0]) % 16 == 0) && (job[3] % 8 == 0);
    if (vec) {
        // all 16 loads of the thread's four chunks first: the pointers may alias as far as the compiler knows, so a rolled form waits
        // for chunk k's stores before it issues chunk k + 1's loads
        f32x4 pq[4], mq[4], vq[4], gq[4];
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const long i = base + (long)(it * 256 + threadIdx.x) * 4;
            if (i < n) { pq[it] = *(const f32x4*)(p + i); mq[it] = *(const f32x4*)(m + i); vq[it] = *(const f32x4*)(v + i); gq[it] = *(const f32x4*)(g + i); }
        }
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const long i = base + (long)(it * 256 + threadIdx.x) * 4;
            if (i >= n) break;
            f32x4 pp = pq[it], mm = mq[it], vv = vq[it];
            const f32x4 gg = gq[it];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float mr = mm[r], vr = vv[r];
                pp[r] = adam_one(pp[r], SCALED ? __fmul_rn(gg[r], coef) : gg[r], mr, vr, a);
                mm[r] = mr;
                vv[r] = vr;
            }
            *(f32x4*)(p + i) = pp;
            *(f32x4*)(m + i) = mm;
            *(f32x4*)(v + i) = vv;
            if (copy) {
                if (copy_f32) *(f32x4*)((float*)copy + i) = pp;
                else *(u32x2*)((bf16_t*)copy + i) = (u32x2){pack2bf(pp[0], pp[1]), pack2bf(pp[2], pp[3])};
            }
        }
    } else {
        long end = base + ADAM_CHUNK;
        end = end < n ? end : n;
        for (long i = base + threadIdx.x; i < end; i += 256) {
            float mr = m[i], vr = v[i];
            const float pn = adam_one(p[i], SCALED ? __fmul_rn(g[i], coef) : g[i], mr, vr, a);
            p[i] = pn;
            m[i] = mr;
            v[i] = vr;
            if (copy) {
                if (copy_f32) ((float*)copy)[i] = pn;
                else ((bf16_t*)copy)[i] = f2bf(pn);
            }
        }
    }
}

// ---------------------------------------------------------------------------------- global gradient norm (clipping)
// Stage 1: block (x, y) sums the squares of chunk x of job y's gradient - the ADAM_CHUNK chunking and thread mapping of
// adam_multi_kernel - in fp32 and in a fixed order: <= 16 products per thread, the 6-step shuffle tree of wave_sum, the four wave
// sums in index order.  One partial per chunk, written with a plain store to partials[chunks of jobs 0 .. y-1 + x]; a job without a
// gradient this step owns no chunks (it contributes exact zeros, and the partials are those of the table without it).  Which block
// writes which word is a function of the two job tables only: no atomics, no dispatch order.
__device__ __forceinline__ long norm_chunks(long n, int64_t grad) { return grad ? (n + ADAM_CHUNK - 1) / ADAM_CHUNK : 0; }

__global__ __launch_bounds__(256) void grad_sqnorm_kernel(const int64_t* __restrict__ table, const int64_t* __restrict__ dynt,
                                                          float* __restrict__ partials) {
    const int64_t* job = table + (long)blockIdx.y * 6;
    const long n = job[4];
    const long base = (long)blockIdx.x * ADAM_CHUNK;
    const float* g = (const float*)dynt[(long)blockIdx.y * 2];
    if (base >= n || g == nullptr) return;
    float acc = 0.f;
    {
        const bool vec = (n % 4 == 0) && ((int64_t)g % 16 == 0);
        if (vec) {
            f32x4 gq[4];
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const long i = base + (long)(it * 256 + threadIdx.x) * 4;
                gq[it] = i < n ? *(const f32x4*)(g + i) : (f32x4){0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int it = 0; it < 4; ++it)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc = fmaf(gq[it][r], gq[it][r], acc);
        } else {
            long end = base + ADAM_CHUNK;
            end = end < n ? end : n;
            for (long i = base + threadIdx.x; i < end; i += 256) acc = fmaf(g[i], g[i], acc);
        }
    }
    // this chunk's slot: the chunks of every job before this one (one strided pass over the table; it overlaps the gradient loads)
    long before = 0;
    for (long j = threadIdx.x; j < (long)blockIdx.y; j += 256) before += norm_chunks(table[j * 6 + 4], dynt[j * 2]);
    __shared__ float ws[4];
    __shared__ long wo[4];
    acc = wave_sum(acc);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o, 64);
    if ((threadIdx.x & 63) == 0) { ws[threadIdx.x >> 6] = acc; wo[threadIdx.x >> 6] = before; }
    __syncthreads();
    if (threadIdx.x == 0) partials[wo[0] + wo[1] + wo[2] + wo[3] + blockIdx.x] = ((ws[0] + ws[1]) + ws[2]) + ws[3];
}

// Stage 2, ONE block: thread t adds partials t, t + 256, ... in index order in double, a fixed LDS tree adds the 256 sums, thread 0
// takes the root and evaluates coef = min(1, max_norm / (total + 1e-6)) in double (NaN propagates through the comparison; total = inf
// gives 0; max_norm = inf gives 1) and rounds once.  result = {total norm, coef, number of gradient elements} as fp32.
__global__ __launch_bounds__(256) void grad_norm_final_kernel(const int64_t* __restrict__ table, const int64_t* __restrict__ dynt,
                                                              long njobs, const float* __restrict__ partials,
                                                              float* __restrict__ result, double max_norm) {
    __shared__ double sd[256];
    __shared__ long sc[256];
    __shared__ double se[256];
    long count = 0;
    double elems = 0.0;
    for (long j = threadIdx.x; j < njobs; j += 256) {
        const long n = table[j * 6 + 4];
        count += norm_chunks(n, dynt[j * 2]);
        if (dynt[j * 2] != 0) elems += (double)n;
    }
    sc[threadIdx.x] = count;
    se[threadIdx.x] = elems;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { sc[threadIdx.x] += sc[threadIdx.x + o]; se[threadIdx.x] += se[threadIdx.x + o]; }
        __syncthreads();
    }
    count = sc[0];
    double acc = 0.0;
    for (long i = threadIdx.x; i < count; i += 256) acc += (double)partials[i];
    sd[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sd[threadIdx.x] += sd[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double total = sqrt(sd[0]);
        const double c = max_norm / (total + 1e-6);
        result[0] = (float)total;
        result[1] = (float)(c > 1.0 ? 1.0 : c);
        result[2] = (float)se[0];
    }
}

// g *= *scale in place (one rounded fp32 multiply, the multiply of adam_multi_kernel<true>), same chunking, both paths.
__global__ __launch_bounds__(256) void scale_multi_kernel(const int64_t* __restrict__ table, const int64_t* __restrict__ dynt,
                                                          const float* __restrict__ scale) {
    const long n = table[(long)blockIdx.y * 6 + 4];
    const long base = (long)blockIdx.x * ADAM_CHUNK;
    float* g = (float*)dynt[(long)blockIdx.y * 2];
    if (base >= n || g == nullptr) return;
    const float coef = *scale;
    if ((n % 4 == 0) && ((int64_t)g % 16 == 0)) {
        f32x4 gq[4];
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const long i = base + (long)(it * 256 + threadIdx.x) * 4;
            if (i < n) gq[it] = *(const f32x4*)(g + i);
        }
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const long i = base + (long)(it * 256 + threadIdx.x) * 4;
            if (i >= n) break;
            f32x4 gg = gq[it];
#pragma unroll
            for (int r = 0; r < 4; ++r) gg[r] = __fmul_rn(gg[r], coef);
            *(f32x4*)(g + i) = gg;
        }
    } else {
        long end = base + ADAM_CHUNK;
        end = end < n ? end : n;
        for (long i = base + threadIdx.x; i < end; i += 256) g[i] = __fmul_rn(g[i], coef);
    }
}

// ---------------------------------------------------------------------------------- gradient accumulation (windows of N micro-batches)
// One micro-step of a window over the Adam job table: job y's accumulator takes this micro-step's gradient, and at the close of the
// window the mean.  Per-call row {grad, mode}: mode 0 = no contribution in the window so far (the accumulator is neither read nor
// written), 1 = first contribution (acc = g: an overwrite, nothing was zeroed), 2 = contributed before (acc = acc + g, or untouched
// when grad is 0).  scale != 1 (the close): every row of mode 1 or 2 is then multiplied by it.  One __fadd_rn per element per
// micro-step in micro-step order, one __fmul_rn at the close: the bits are those of ((g1 + g2) + ...) * scale in fp32.  The chunking
// and thread mapping of adam_multi_kernel, every load of a thread before its first store, no atomics.
__global__ __launch_bounds__(256) void grad_accum_kernel(const int64_t* __restrict__ table, const int64_t* __restrict__ dynt,
                                                         const int64_t* __restrict__ accp, float scale) {
    const long n = table[(long)blockIdx.y * 6 + 4];
    const long base = (long)blockIdx.x * ADAM_CHUNK;
    const float* g = (const float*)dynt[(long)blockIdx.y * 2];
    const int64_t mode = dynt[(long)blockIdx.y * 2 + 1];
    const bool first = mode == 1;
    const bool scaled = scale != 1.0f;
    if (base >= n || mode == 0 || (g == nullptr && (first || !scaled))) return;
    float* acc = (float*)accp[blockIdx.y];
    if ((n % 4 == 0) && (((int64_t)g | (int64_t)acc) % 16 == 0)) {
        f32x4 aq[4], gq[4];
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const long i = base + (long)(it * 256 + threadIdx.x) * 4;
            if (i < n) {
                if (!first) aq[it] = *(const f32x4*)(acc + i);
                if (g) gq[it] = *(const f32x4*)(g + i);
            }
        }
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const long i = base + (long)(it * 256 + threadIdx.x) * 4;
            if (i >= n) break;
            f32x4 aa;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float x = first ? gq[it][r] : (g ? __fadd_rn(aq[it][r], gq[it][r]) : aq[it][r]);
                if (scaled) x = __fmul_rn(x, scale);
                aa[r] = x;
            }
            *(f32x4*)(acc + i) = aa;
        }
    } else {
        long end = base + ADAM_CHUNK;
        end = end < n ? end : n;
        for (long i = base + threadIdx.x; i < end; i += 256) {
            float x = first ? g[i] : (g ? __fadd_rn(acc[i], g[i]) : acc[i]);
            if (scaled) x = __fmul_rn(x, scale);
            acc[i] = x;
        }
    }
}

// ---------------------------------------------------------------------------------- exponential moving average of the weights
// Behind the Adam launches of an update: job y's average moves towards its parameter, ema = ema + weight * (p - ema), as three
// rounded fp32 operations (__fsub_rn, __fmul_rn, __fadd_rn: no fused multiply-add, so the bits are those of torch's
// e + w * (p - e) on CPU tensors).  Only the parameter pointer (column 0) and n (column 4) of the Adam job table are read; there is
// no per-step row: a job without a gradient in this update (LayerDrop) still averages.  The chunking and thread mapping of
// adam_multi_kernel, every load of a thread before its first store, no atomics.
// (the build runs with -ffp-contract=fast, under which the back end fuses a * b + c whatever the source says, and the __f*_rn
// spellings are plain operators here: the empty asm makes the rounded product opaque, so the add cannot absorb the multiply)
__device__ __forceinline__ float ema_one(float e, float p, float weight) {
    float s = __fmul_rn(weight, __fsub_rn(p, e));
    asm volatile("" : "+v"(s));
    return __fadd_rn(e, s);
}

__global__ __launch_bounds__(256) void ema_multi_kernel(const int64_t* __restrict__ table, const int64_t* __restrict__ emap,
                                                        float weight) {
    const int64_t* job = table + (long)blockIdx.y * 6;
    const long n = job[4];
    const long base = (long)blockIdx.x * ADAM_CHUNK;
    if (base >= n) return;
    const float* p = (const float*)job[0];
    float* e = (float*)emap[blockIdx.y];
    if ((n % 4 == 0) && ((job[0] | (int64_t)e) % 16 == 0)) {
        f32x4 pq[4], eq[4];
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const long i = base + (long)(it * 256 + threadIdx.x) * 4;
            if (i < n) { pq[it] = *(const f32x4*)(p + i); eq[it] = *(const f32x4*)(e + i); }
        }
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const long i = base + (long)(it * 256 + threadIdx.x) * 4;
            if (i >= n) break;
            f32x4 ee = eq[it];
#pragma unroll
            for (int r = 0; r < 4; ++r) ee[r] = ema_one(ee[r], pq[it][r], weight);
            *(f32x4*)(e + i) = ee;
        }
    } else {
        long end = base + ADAM_CHUNK;
        end = end < n ? end : n;
        for (long i = base + threadIdx.x; i < end; i += 256) {
            e[i] = ema_one(e[i], p[i], weight);
        }
    }
}

// Exchanges job y's parameter and its average element for element (evaluation on the averaged weights and back: the pointers stay,
// so job tables and captured graphs remain valid).  Same table columns, chunking, paths and load-before-store order as above.
__global__ __launch_bounds__(256) void swap_multi_kernel(const int64_t* __restrict__ table, const int64_t* __restrict__ emap) {
    const int64_t* job = table + (long)blockIdx.y * 6;
    const long n = job[4];
    const long base = (long)blockIdx.x * ADAM_CHUNK;
    if (base >= n) return;
    float* p = (float*)job[0];
    float* e = (float*)emap[blockIdx.y];
    if ((n % 4 == 0) && ((job[0] | (int64_t)e) % 16 == 0)) {
        f32x4 pq[4], eq[4];
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const long i = base + (long)(it * 256 + threadIdx.x) * 4;
            if (i < n) { pq[it] = *(const f32x4*)(p + i); eq[it] = *(const f32x4*)(e + i); }
        }
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const long i = base + (long)(it * 256 + threadIdx.x) * 4;
            if (i >= n) break;
            *(f32x4*)(p + i) = eq[it];
            *(f32x4*)(e + i) = pq[it];
        }
    } else {
        long end = base + ADAM_CHUNK;
        end = end < n ? end : n;
        for (long i = base + threadIdx.x; i < end; i += 256) {
            const float pp = p[i], ee = e[i];
            p[i] = ee;
            e[i] = pp;
        }
    }
}

}  // namespace

static int adam_launch(const char* who, const int64_t* table_dev, const int64_t* dyn_dev, int64_t njobs, int64_t max_n, float lr,
                       float beta1, float beta2, float eps, float weight_decay, const float* grad_scale_dev, bool scaled, void* stream) {
    APTAI_REQUIRE(table_dev && dyn_dev && njobs > 0 && njobs <= 65535 && max_n > 0, "%s: bad arguments", who);
    APTAI_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "%s: betas must lie in [0, 1)", who);
    APTAI_REQUIRE(!scaled || grad_scale_dev, "%s: grad_scale_dev is null", who);
    AdamArgs a;
    a.table = table_dev;
    a.dyn = dyn_dev;
    a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.weight_decay = weight_decay;
    a.bc1 = a.bc2_sqrt = 1.f;
    const dim3 grid((unsigned)ceil_div(max_n, ADAM_CHUNK), (unsigned)njobs);
    if (scaled) APTAI_LAUNCH(adam_multi_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a, grad_scale_dev);
    else APTAI_LAUNCH(adam_multi_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a, (const float*)nullptr);
    APTAI_CHECK_LAUNCH("adam_multi_kernel");
    return APTAI_OK;
}

extern "C" int aptai_adam_multi(const int64_t* table_dev, const int64_t* dyn_dev, int64_t njobs, int64_t max_n, float lr, float beta1,
                                float beta2, float eps, float weight_decay, void* stream) {
    return adam_launch("aptai_adam_multi", table_dev, dyn_dev, njobs, max_n, lr, beta1, beta2, eps, weight_decay, nullptr, false, stream);
}

extern "C" int aptai_adam_multi_scaled(const int64_t* table_dev, const int64_t* dyn_dev, int64_t njobs, int64_t max_n, float lr,
                                       float beta1, float beta2, float eps, float weight_decay, const float* grad_scale_dev,
                                       void* stream) {
    return adam_launch("aptai_adam_multi_scaled", table_dev, dyn_dev, njobs, max_n, lr, beta1, beta2, eps, weight_decay,
                       grad_scale_dev, true, stream);
}

extern "C" int aptai_grad_sqnorm_multi(const int64_t* table_dev, const int64_t* dyn_dev, int64_t njobs, int64_t max_n,
                                       float* partials_dev, float* result_dev, double max_norm, void* stream) {
    APTAI_REQUIRE(table_dev && dyn_dev && partials_dev && result_dev && njobs > 0 && njobs <= 65535 && max_n > 0,
                  "aptai_grad_sqnorm_multi: bad arguments");
    APTAI_REQUIRE(max_norm >= 0.0, "aptai_grad_sqnorm_multi: max_norm must be >= 0 (inf measures without clipping)");
    APTAI_LAUNCH(grad_sqnorm_kernel, dim3((unsigned)ceil_div(max_n, ADAM_CHUNK), (unsigned)njobs), dim3(256), 0, (hipStream_t)stream,
                 table_dev, dyn_dev, partials_dev);
    APTAI_CHECK_LAUNCH("grad_sqnorm_kernel");
    APTAI_LAUNCH(grad_norm_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, table_dev, dyn_dev, (long)njobs,
                 (const float*)partials_dev, result_dev, max_norm);
    APTAI_CHECK_LAUNCH("grad_norm_final_kernel");
    return APTAI_OK;
}

extern "C" int aptai_scale_multi(const int64_t* table_dev, const int64_t* dyn_dev, int64_t njobs, int64_t max_n, const float* scale_dev,
                                 void* stream) {
    APTAI_REQUIRE(table_dev && dyn_dev && scale_dev && njobs > 0 && njobs <= 65535 && max_n > 0, "aptai_scale_multi: bad arguments");
    APTAI_LAUNCH(scale_multi_kernel, dim3((unsigned)ceil_div(max_n, ADAM_CHUNK), (unsigned)njobs), dim3(256), 0, (hipStream_t)stream,
                 table_dev, dyn_dev, scale_dev);
    APTAI_CHECK_LAUNCH("scale_multi_kernel");
    return APTAI_OK;
}

extern "C" int aptai_grad_accum_multi(const int64_t* table_dev, const int64_t* dyn_dev, const int64_t* acc_dev, int64_t njobs,
                                      int64_t max_n, float scale, void* stream) {
    APTAI_REQUIRE(table_dev && dyn_dev && acc_dev && njobs > 0 && njobs <= 65535 && max_n > 0, "aptai_grad_accum_multi: bad arguments");
    APTAI_REQUIRE(scale > 0.f && scale <= 3.402823466e38f, "aptai_grad_accum_multi: scale must be finite and positive (1 / micro-steps)");
    APTAI_LAUNCH(grad_accum_kernel, dim3((unsigned)ceil_div(max_n, ADAM_CHUNK), (unsigned)njobs), dim3(256), 0, (hipStream_t)stream,
                 table_dev, dyn_dev, acc_dev, scale);
    APTAI_CHECK_LAUNCH("grad_accum_kernel");
    return APTAI_OK;
}

extern "C" int aptai_ema_multi(const int64_t* table_dev, const int64_t* ema_dev, int64_t njobs, int64_t max_n, float weight,
                               void* stream) {
    APTAI_REQUIRE(table_dev && ema_dev && njobs > 0 && njobs <= 65535 && max_n > 0, "aptai_ema_multi: bad arguments");
    APTAI_REQUIRE(weight > 0.f && weight <= 1.f, "aptai_ema_multi: weight must lie in (0, 1] (1 - decay of this update)");
    APTAI_LAUNCH(ema_multi_kernel, dim3((unsigned)ceil_div(max_n, ADAM_CHUNK), (unsigned)njobs), dim3(256), 0, (hipStream_t)stream,
                 table_dev, ema_dev, weight);
    APTAI_CHECK_LAUNCH("ema_multi_kernel");
    return APTAI_OK;
}

extern "C" int aptai_swap_multi(const int64_t* table_dev, const int64_t* ema_dev, int64_t njobs, int64_t max_n, void* stream) {
    APTAI_REQUIRE(table_dev && ema_dev && njobs > 0 && njobs <= 65535 && max_n > 0, "aptai_swap_multi: bad arguments");
    APTAI_LAUNCH(swap_multi_kernel, dim3((unsigned)ceil_div(max_n, ADAM_CHUNK), (unsigned)njobs), dim3(256), 0, (hipStream_t)stream,
                 table_dev, ema_dev);
    APTAI_CHECK_LAUNCH("swap_multi_kernel");
    return APTAI_OK;
}
