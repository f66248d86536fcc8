/* aptai_hip.h — C ABI of libaptai_hip.so: the MI355X (gfx950) kernels behind APTAI's hot path.
 *
 * The reference (tobwei/APTAI) has no native/FFI layer: its hot path is Python calling torch/ATen operators
 * through HuggingFace's Wav2Vec2Model.  Each entry point below therefore cites the reference
 * *operator call site* it replaces ("HF:n" = transformers/models/wav2vec2/modeling_wav2vec2.py line n).
 *
 * Conventions
 *  - the caller owns every buffer; pointers are raw DEVICE pointers unless a parameter says "host";
 *    nothing here allocates device memory (workspaces are caller-provided, sized by *_workspace_bytes);
 *  - all launches go to the hipStream_t passed as `stream` (void*); no internal synchronisation;
 *  - return 0 (APTAI_OK) or a negative aptai_status; aptai_last_error() gives a thread-local message;
 *  - "bf16" = raw bfloat16 (uint16_t storage); activations are row-major [rows][cols] with frames as rows
 *    (channels-last); statistics, biases, norm parameters, losses and gradients of parameters are fp32;
 *  - integer outputs (lengths, argmax / alignment indices) are int64 and bit-exact by construction.
 */
#ifndef APTAI_HIP_H
#define APTAI_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    APTAI_OK = 0,
    APTAI_ERR_INVALID = -1,  /* bad argument / unsupported shape */
    APTAI_ERR_LAUNCH = -2,   /* HIP launch failure */
    APTAI_ERR_NO_DEVICE = -3
} aptai_status;

const char* aptai_last_error(void);
int aptai_version(void);
/* device sanity: returns APTAI_OK iff a gfx950 device is current; fills name (<=63 chars) if non-null */
int aptai_device_check(char* name, int name_len);
/* Per-step dropout salt, bound to ONE stream: device pointer to two uint32 words that every seeded kernel launched (or
 * captured) on `stream` XORs into its dropout seed; null clears the binding.  A captured hipGraph thereby draws fresh masks
 * on each replay; forward and backward of one step stay consistent.  Launches on other streams are unaffected (no
 * process-global state: two runners / two models on two streams are independent).  The caller keeps the two words alive
 * until it clears the binding. */
int aptai_set_seed_salt(void* stream, const void* device_ptr_2xu32);
/* Per-step frame bounds, bound to ONE stream like the salt: device pointer to two int32 words {frames of the first conv layer that
 * count for its GroupNorm statistics (HF:317-323), frames that exist for LowPassFilterLayer's zero padding (models/modules.py:46-61)};
 * null clears the binding.  The reference pads every batch to ITS OWN longest utterance (train/train_aptai.py:268-285), and both
 * operations see that padded length; a hipGraph captured for a longer bucket length replays with the bounds of the batch it is fed
 * (aptai_conv0_fwd / aptai_conv0_bwd in group mode and aptai_lowpass_fir read them), so it equals the eager run on the batch's
 * own shape.  The caller keeps the two words alive until it clears the binding. */
int aptai_set_frame_bounds(void* stream, const void* device_ptr_2xi32);

/* ------------------------------------------------------------------------------------------------ GEMM
 * C[M,N] = A . B^T with fp32 accumulation (MFMA), replacing nn.Linear / nn.Conv1d(k>1 as implicit GEMM):
 *   q/k/v/out_proj HF:495-498,522-527,546; FFN HF:556-572; feature projection HF:429-434;
 *   conv layers 1..6 HF:260-266 (A rows overlap: lda = stride*C_in < K = kernel*C_in, channels-last frames).
 * a_kmajor/b_kmajor: operand stored [K][rows] instead of [rows][K] (dgrad: B K-major; wgrad: both).
 * Epilogue order: alpha, +bias, (store out_pre), GELU, dropout, *gelu'(aux), +residual, cast. */
enum {
    APTAI_EPI_BIAS = 1,
    APTAI_EPI_GELU = 2,      /* GELU in place of ACT2FN["gelu"] (HF:267-272,560): x * sigmoid(x (a1 + a3 x^2 + a5 x^4)), a logistic fit of the
                              * normal CDF: |y - erf form| <= 3.3e-5, |y' - exact| <= 1.3e-4 (below the bf16 grid of the stored output) */
    APTAI_EPI_RESIDUAL = 4,  /* += residual[m*ldr+n] (bf16) */
    APTAI_EPI_DROPOUT = 8,   /* counter-based mask from (seed, m*N+n); scaled by 1/(1-p) */
    APTAI_EPI_DGELU = 16,    /* *= gelu'(aux[m*ldaux+n]) — backward of the FFN activation */
    APTAI_EPI_ALPHA = 32,
    APTAI_EPI_PRE_DGELU = 64, /* with EPI_GELU: out_pre receives dropmask/(1-p) * gelu'(pre-activation) instead of the pre-activation */
    APTAI_EPI_MUL_AUX = 128,  /* *= aux[m*ldaux+n] (bf16): the backward partner of EPI_PRE_DGELU */
    APTAI_EPI_RESIDUAL_F32 = 256, /* fp32 output only (tile 64 / 128 / 192): += residual[m*ldr+n] read as FP32 - the residual stream of the
                                   * inference-only encoder kept in fp32 (HF:594-601: hidden_states = attn_residual + hidden_states) */
    APTAI_EPI_BIAS_ROW = 1024,    /* out_f32 launches only: bias is indexed by the output ROW (bias[m], length M) - a product evaluated transposed,
                                   * C^T = W . X^T, carries its Linear bias along the rows (the exact mode's V^T projection) */
    APTAI_EPI_SPLIT_OUT = 512     /* out_f32 launches on tile 128 / 192 / 256 (exact-index mode): the fp32 result [-> erf GELU with EPI_GELU] leaves as
                                   * `split_out_pieces` bf16 pieces in the activation-side layout of aptai_split_f32, [m][N/64][piece][64],
                                   * C = bf16*, ldc (and the C batch strides) in bf16 elements, ldc >= pieces * N: the next split-operand
                                   * GEMM's A operand, written once instead of an fp32 store, a re-read and a split pass */
};

typedef struct {
    const void* A; int64_t lda;     /* bf16 */
    const void* B; int64_t ldb;     /* bf16 */
    void* C; int64_t ldc;           /* bf16, or fp32 when out_f32 */
    int64_t M, N, K;                /* K % 64 == 0, N % 8 == 0 */
    int a_kmajor, b_kmajor, out_f32;
    int flags;
    const float* bias;              /* [N] fp32 */
    const void* residual; int64_t ldr;
    void* out_pre;                  /* optional bf16 [M][ldc]: value before GELU (saved for backward) */
    const void* aux; int64_t ldaux;
    float alpha;
    float dropout_p; uint64_t seed;
    int split_k;                    /* fp32 output only: K split into slabs in `workspace`, then reduced */
    int accumulate;                 /* fp32 output only: C += result */
    void* workspace; int64_t workspace_bytes;
    /* optional 2-level batching (grouped positional conv: outer = utterance, inner = group); strides in elements */
    int batch_outer, batch_inner;
    int64_t batch_stride_a[2], batch_stride_b[2], batch_stride_c[2], batch_stride_bias[2], batch_stride_res[2],
        batch_stride_aux[2];
    int tile;                       /* 0 = auto, 64 = 64x128 tile (3 blocks/CU, K-contiguous A), 128 = 128x128 tile kernel (2 blocks/CU), 192 = 128x192 tile, 3-stage ring
                                       (1 block/CU), 256 = 256x256 deep-pipelined kernel, 448 = 256x192 tile (bf16 out, K-contiguous A, one problem), 257 = the 256x256 tile as a persistent stream-K
                                       kernel (one workgroup per CU, equal shares of (tile, K-tile) iterations; needs sk_workspace) */
    int colscale_n; float colscale; /* bf16 output: columns [0, colscale_n) *= colscale after alpha / bias (colscale_n % 8 == 0).  The fused
                                       q|k|v projection (HF:495-498) hands the attention kernels Q already multiplied by
                                       head_dim^-0.5 * log2(e) (HF:522 applies the scaling to the projected query too), rounded once */
    void* sk_workspace;             /* optional, aptai_gemm_sk_workspace_bytes() bytes, ZEROED ONCE by the caller and then owned by ONE stream:
                                       fp32 partial-tile slabs + ready flags (self-cleaning) + status word of the stream-K kernel.  Tile 257 is
                                       opt-in only: without the workspace it is refused, and the auto rule never picks it */
    int64_t sk_workspace_bytes;
    int split_out_pieces;           /* with APTAI_EPI_SPLIT_OUT: 3 or 6 */
    int split_out_bcol;             /* with APTAI_EPI_SPLIT_OUT: output columns n >= split_out_bcol are written in the WEIGHT-side piece order
                                       (hi lo hi | hi mid hi mid low hi), columns below it in the activation-side order; N (or more) = all
                                       activation-side.  A fused q|k projection hands Q (A operand of Q K^T) and K (its B operand) over at once */
} aptai_gemm_desc;

int aptai_gemm_bf16(const aptai_gemm_desc* desc, void* stream);
/* n (<= 8) independent problems of ONE operand layout / output type in a single launch (no batching, split-K or
 * accumulate).  Made for the per-layer weight and bias gradients of the encoder backward, which autograd computes as
 * separate `grad_out.t() @ input` / `grad_out.sum(0)` kernels behind HF:478-480,575-654 (nn.Linear backward): together
 * their full-K tiles fill the 256 CUs once, where each alone needs split-K slabs and a reduce pass.  A bias gradient is
 * the problem M = 8, A = ones[K][8] (K-major), row 0 of the [8][N] fp32 result. */
int aptai_gemm_bf16_grouped(const aptai_gemm_desc* descs, int n, void* stream);
/* The same launch with an optional fp32 row-sum output per problem: rowsums is null or an array of n device pointers, null = none.
 * rowsums[i][m] = sum_k A_i[k][m] for the M_i output rows of problem i, i.e. the column sums of a K-major A: with A = dY of a weight
 * gradient dW = dY^T X that is the bias gradient, so it needs no ones[K][8] problem of its own.  The tiles of the problem's first
 * tile column form it from the A fragments they already hold, with one more MFMA per fragment against a register of ones, in the K
 * order of the tile's own accumulation (no atomics: same inputs, same bits; the same bits as row 0 of the ones problem).  Each of the
 * M_i floats is written once; nothing beyond them is touched.  Refused with APTAI_ERR_INVALID: a row-sum pointer on a problem whose
 * operands are not both K-major, whose output is not fp32, or that asks for split-K slabs (each slab would hold a partial sum).
 * aptai_gemm_bf16_grouped is this entry with rowsums = null. */
int aptai_gemm_bf16_grouped_rowsum(const aptai_gemm_desc* descs, float* const* rowsums, int n, void* stream);
/* What aptai_gemm_bf16 would launch for `desc` in this process (environment knobs included), without touching the device: the same
 * validation and the same planner, so a refused descriptor returns the status and aptai_last_error() text of aptai_gemm_bf16. */
typedef struct {
    int tile;                       /* kernel, as in aptai_gemm_desc.tile (never 0) */
    int nbatch, nsplit;             /* grid y (batches) and z (split-K slabs as launched) */
    int ktiles_per_split;           /* 64-deep K-tiles per slab */
    int raster_gm;                  /* tile rows per raster group, 0 = row-major walk */
    int64_t split_n;                /* 0 = one launch; else two launches (APTAI_GEMM_SPLITN=1): columns [0, split_n) as `tile` (256),
                                       columns [split_n, N) as 128-row tiles */
} aptai_gemm_plan_info;
int aptai_gemm_plan(const aptai_gemm_desc* desc, aptai_gemm_plan_info* out);
int64_t aptai_gemm_workspace_bytes(int64_t M, int64_t N, int split_k);
/* Stream-K workspace (independent of the problem: one 256 x 256 fp32 slab per CU + flags) and its status word: non-zero after a
 * launch in which a bounded wait for another workgroup's slab gave up (that launch's output is then incomplete; never a hang).
 * aptai_gemm_sk_status copies the word to the host behind everything queued on `stream` (synchronises) and clears it. */
int64_t aptai_gemm_sk_workspace_bytes(void);
int aptai_gemm_sk_status(void* sk_workspace, void* stream, int* status_out);

/* ------------------------------------------------------------------------------------------------ exact (fp32-class) inference path
 * Wav2Vec2Model.set_encoder_precision("f32x3" | "f32x6"): the frozen recogniser inside Force_APTAI (models/force_aptai.py:60-78,
 * 124-127, inference only) with every matrix product at fp32-class accuracy, so that the alignment argmax (:148-161) and the
 * best-path decode see the reference's fp32 scores.  aptai_split_f32 turns an fp32 operand [rows][cols] into bf16 pieces in the
 * K-tile-interleaved layout [row][cols/64][pieces][64] (pattern 0 = activation side: hi,hi,lo | hi,hi,mid,mid,hi,low; pattern 1 =
 * weight side: hi,lo,hi | hi,mid,hi,mid,low,hi), which aptai_gemm_bf16 (NT, fp32 output, K' = pieces * K, lda' = pieces * lda)
 * multiplies as hi.hi + hi.lo + lo.hi (+ mid.mid + hi.low + low.hi): relative error ~2^-17 (3 pieces) / ~2^-24 (6 pieces) with
 * fp32 accumulation.  act = 1 applies the erf-form GELU (ACT2FN["gelu"], HF:267-272,560) before the split. */
int aptai_split_f32(const float* x, int64_t ldx, int64_t rows, int64_t cols, int pattern, int pieces, int act, void* out, int64_t ldo,
                    void* stream);
/* y = [res +] act(x + bias) in fp32 (act 0 none, 1 erf GELU); with lens (int32 [rows / rows_per_b]) rows t >= lens[b] of each block
 * of rows_per_b rows are zeroed (padded frames, HF:678-681).  In place (y == x) allowed. */
int aptai_bias_act_res_f32(const float* x, int64_t ldx, const float* bias, const float* res, int64_t ldr, float* y, int64_t ldy,
                           int64_t rows, int64_t cols, int act, const int32_t* lens, int64_t rows_per_b, void* stream);
/* softmax over keys, in place on fp32 scores s[B][heads][Tp][Tp]; keys >= lens[b] get probability 0 (HF:452-461 under the
 * finfo.min key mask of HF:1018-1036). */
int aptai_softmax_rows_f32(float* s, const int32_t* lens, int64_t B, int64_t heads, int64_t Tp, void* stream);
/* The same masked softmax written straight into the split (activation-side) layout [row][Tp/64][piece][64] of its probabilities - the A
 * operand of the exact attention's P . V product (aptai_amd/wav2vec2.py _exact_attention; replaces torch softmax at HF:452-461 followed by
 * aptai_split_f32: the fp32 probabilities are never stored).  s fp32 [B][heads][Tp][Tp]; out bf16, row pitch ldo >= pieces * Tp. */
int aptai_softmax_split_f32(const float* s, const int32_t* lens, int64_t B, int64_t heads, int64_t Tp, int pieces, void* out, int64_t ldo,
                            void* stream);
/* The whole attention core of the exact-index mode in ONE launch: softmax(Q K^T * scale + key mask) V per (utterance, head), every product
 * as the 3 (pieces = 3, "f32x3") or 6 (pieces = 6, "f32x6") leading bf16 piece products accumulated in fp32, the scores and probabilities
 * never stored (replaces HF:452-461 on the path of models/force_aptai.py:148-161 whose argmax indices must be the reference's; round 4's
 * three launches - aptai_gemm_bf16 scores, aptai_softmax_split_f32, aptai_gemm_bf16 P . V - moved ~0.8 GB per layer at 16 x 10 s).
 * qkv_split bf16 [B*Tp][ld >= 3 * pieces * H]: thirds Q | K | V of pieces * H columns, head h = columns [64 * pieces * h, +64 * pieces)
 * of its third as [slot][64]; Q in the activation-side slot order, K and V in the weight-side order - what one aptai_gemm_bf16 launch with
 * APTAI_EPI_SPLIT_OUT, split_out_pieces = pieces and split_out_bcol = H writes for the concatenated q|k|v weight.  lens int32 [B]: keys
 * >= lens[b] get probability 0, query rows beyond it are computed like the reference's.  ctx_split bf16 [B*Tp][ldo >= pieces * H] in the
 * activation-side split layout: the out-projection's A operand.  Tp % 128 == 0, head_dim 64.  Inference only (no dropout, no backward). */
int aptai_attention_exact_fwd(const void* qkv_split, int64_t ld, const int32_t* lens, void* ctx_split, int64_t ldo, int64_t B, int64_t Tp,
                              int64_t H, int64_t heads, int pieces, float scale, void* stream);
/* Conv1d(1,512,10,5) + GroupNorm / LayerNorm + erf GELU with FP32 output [B][T_alloc][512] (HF:260-323); `stats` = the (mean, rstd)
 * block [B][2][512] of aptai_conv0_fwd in group mode (mode 0), unused in layer mode (mode 1). */
int aptai_conv0_fwd_f32(const float* audio, int64_t B, int64_t S, const float* weight, const float* bias, const float* gamma,
                        const float* beta, int mode, float eps, float* out, int64_t T_real, int64_t T_alloc, const float* stats,
                        void* stream);
/* The same layer with its result written as split bf16 pieces [B][T_alloc][512 / 64][piece][64] - the A operand of the exact mode's second
 * conv layer (round 4: the 1 GB fp32 intermediate at 16 x 10 s is never stored).  Frames in [T_real, T_alloc) are written as zeros. */
int aptai_conv0_fwd_split(const float* audio, int64_t B, int64_t S, const float* weight, const float* bias, const float* gamma,
                          const float* beta, int mode, float eps, void* out_split, int pieces, int64_t T_real, int64_t T_alloc,
                          const float* stats, void* stream);

/* ------------------------------------------------------------------------------------------------ LayerNorm
 * y = (x - mean) * rstd * gamma + beta over the channel axis (cols in {256,512,768,1024}), one wave per row.
 * Replaces nn.LayerNorm at HF:288-299 (conv layers, "layer" mode; gelu_after=1 fuses the GELU of HF:299),
 * HF:425-431, HF:587-601 / 622-644, HF:691 / 791 and models/modules.py:134,151.  x,y bf16; mean/rstd fp32 (may be null). */
int aptai_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                        int64_t rows, int64_t cols, float eps, int gelu_after, void* stream);
/* dx = LN'(dy) [+ dres]; optional dx_drop = dropout-masked copy of dx (mask of (seed, element index), for the
 * branch that went through nn.Dropout, HF:591,628); dgamma/dbeta fp32 [cols] (overwritten). */
/* nn.LayerNorm forward on an FP32 row (the fp32 residual stream of the inference-only encoder): y_bf16 and / or y_f32 receive the
 * normalised row (bf16 for the next GEMM operand, fp32 for the next residual add).  cols in {256, 512, 768, 1024}. */
int aptai_layernorm_fwd_f32in(const float* x, const float* gamma, const float* beta, void* y_bf16, float* y_f32, int64_t rows,
                              int64_t cols, float eps, void* stream);
/* The same LayerNorm with its result ALSO written as split bf16 pieces [rows][cols / 64][piece][64] (activation-side order): the A operand of
 * the exact mode's next split-operand product, without a split pass of its own.  y_f32 may be null. */
int aptai_layernorm_fwd_f32in_split(const float* x, const float* gamma, const float* beta, float* y_f32, void* y_split, int pieces,
                                    int64_t rows, int64_t cols, float eps, void* stream);
int aptai_layernorm_bwd(const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma,
                        const void* dres, void* dx, void* dx_drop, float dropout_p, uint64_t seed, float* dgamma,
                        float* dbeta, void* workspace, int64_t rows, int64_t cols, const float* beta_if_gelu_after,
                        void* stream);   /* beta_if_gelu_after != null: dy is the gradient of gelu(LN(x)) (conv stack, HF:299) */
int64_t aptai_layernorm_bwd_workspace_bytes(int64_t rows, int64_t cols);
/* The dgamma / dbeta reductions of MANY aptai_layernorm_bwd calls (each called with dgamma = dbeta = null, its workspace kept) in one
 * launch: table_dev = device int64 [njobs][5] = {workspace of that call, dgamma | 0, dbeta | 0, blocks = workspace_bytes / (8 * cols),
 * cols}; max_cols = the widest job.  Replaces the per-call finalisation behind nn.LayerNorm's parameter gradients (HF:587-601). */
int aptai_layernorm_bwd_finalize_multi(const int64_t* table_dev, int64_t njobs, int64_t max_cols, void* stream);

/* ------------------------------------------------------------------------------------------------ attention
 * softmax(Q K^T * scale + key-padding mask) V per head (head_dim 64), flash-style, replacing HF:452-461 / sdpa
 * as called from HF:522-546, and its backward.  qkv [B*Tp][3H] bf16; lens int32 [B] valid frames (keys beyond are
 * masked, HF:678-688); Tp % 128 == 0; ctx [B*Tp][H] bf16; lse2 fp32 [B][heads][Tp] (log2-domain log-sum-exp).
 * dropout_p: attention-probability dropout (HF:458), mask from (seed, (b,h,q,k)).
 * ctx_f32 (optional, [B*Tp][H] fp32): unrounded context; the backward's delta = rowsum(dO*O) is a small-difference term
 * (dS = P*(dP - delta)) whose bf16 rounding would otherwise dominate the q/k gradients when attention is diffuse.
 * q_prescaled != 0: the Q third of qkv already carries scale * log2(e) (aptai_gemm_desc.colscale of the fused q|k|v projection):
 * the scores arrive in the exp2 domain, the backward starts its S / dP accumulators at -lse2 / -delta, and dqkv's Q third is
 * still the gradient with respect to the UNSCALED projection output (what the projection's own backward expects). */
int aptai_attention_fwd(const void* qkv, const int32_t* lens, void* ctx, float* lse2, float* ctx_f32, int64_t B, int64_t Tp,
                        int64_t H, int64_t heads, float scale, float dropout_p, uint64_t seed, int q_prescaled, void* stream);
/* delta_ws: fp32 [B][heads][Tp] scratch.  dctx_zero_beyond_len=1 lets the kernel skip query rows >= lens[b]
 * (their incoming gradient is exactly zero in the models: no loss term touches padded frames). */
int aptai_attention_bwd(const void* qkv, const int32_t* lens, const void* ctx, const float* ctx_f32, const void* dctx,
                        const float* lse2, float* delta_ws, void* dqkv, int64_t B, int64_t Tp, int64_t H, int64_t heads, float scale,
                        float dropout_p, uint64_t seed, int dctx_zero_beyond_len, int q_prescaled, void* stream);

/* The attention probabilities the fused forward never writes (HF eager_attention_forward's second result, output_attentions=True),
 * rebuilt from what it saved.  qkv, lens, scale, dropout_p, seed, q_prescaled exactly as given to aptai_attention_fwd, lse2 as that call
 * wrote it.  probs fp32 [B][heads][Tp][Tp] (row pitch Tp, 16-byte aligned; callers view [:, :, :T, :T]): the softmax AFTER dropout,
 * keep * P / (1 - p) with the keep mask the fused kernels used (plain softmax when dropout_p == 0); key columns >= lens[b] are exactly
 * 0, query rows >= lens[b] are computed like all others.  One QK^T product and one streaming write, no row reduction. */
int aptai_attention_probs_fwd(const void* qkv, const int32_t* lens, const float* lse2, float* probs, int64_t B, int64_t Tp, int64_t H,
                              int64_t heads, float scale, float dropout_p, uint64_t seed, int q_prescaled, void* stream);
/* Its backward.  dprobs fp32, layout of probs: gradient of the loss with respect to the RETURNED tensor (all Tp query rows are read;
 * key columns >= lens[b] are ignored).  dS = P (dP - rowsum(dP P)) with dP = keep * dprobs / (1 - p); dQ = scale dS K and
 * dK = scale dS^T Q go to the Q and K thirds of dqkv [B*Tp][3H] bf16, the V third is not touched.  accumulate != 0 adds them to what
 * the thirds hold (what aptai_attention_bwd wrote for the same layer: sum in fp32, one rounding; every element is owned by one lane,
 * so same inputs give the same bits), accumulate == 0 overwrites them; gradients of keys >= lens[b] are exactly zero either way.
 * q_prescaled != 0: the Q third of dqkv is the gradient with respect to the UNSCALED projection output, as for aptai_attention_bwd.
 * rowsum_ws: fp32 [B][heads][Tp] scratch. */
int aptai_attention_probs_bwd(const void* qkv, const int32_t* lens, const float* lse2, const float* dprobs, float* rowsum_ws, void* dqkv,
                              int64_t B, int64_t Tp, int64_t H, int64_t heads, float scale, float dropout_p, uint64_t seed,
                              int q_prescaled, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------------ parameter prep
 * fp32 master parameters -> bf16 compute copies (and the layouts the kernels want). */
int aptai_cast_f32_to_bf16(const float* src, void* dst, int64_t rows, int64_t cols, int64_t ld_dst, void* stream);
/* Many casts in one launch.  table_dev: device int64 [njobs][4] = {src fp32 ptr, dst ptr, n, kind}; n % 8 == 0, both
 * pointers 32-/16-byte aligned; kind 0 = fp32 -> bf16, 1 = fp32 -> fp32 copy (packs q/k/v biases); max_n = largest n. */
int aptai_cast_multi(const int64_t* table_dev, int64_t njobs, int64_t max_n, void* stream);
/* torch.optim.Adam step (train/train_aptai.py:350-356, 443) for many tensors in one launch.  table_dev: device int64
 * [njobs][6] = {param, exp_avg, exp_avg_sq, copy_dst or 0, n, copy_kind (0 = bf16, 1 = fp32)} (static across steps);
 * dyn_dev: device int64 [njobs][2] = {grad or 0 (no gradient this step: the job is skipped), step count of this update >= 1}
 * (rewritten every step).  All tensors fp32 with n elements; copy_dst receives the updated parameter (the compute copy the
 * forward reads).  Bias corrections 1 - beta^step are evaluated per job in double, as torch does on the host. */
int aptai_adam_multi(const int64_t* table_dev, const int64_t* dyn_dev, int64_t njobs, int64_t max_n, float lr, float beta1,
                     float beta2, float eps, float weight_decay, void* stream);
/* Global-norm gradient clipping.  The three entries below replace `torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)`
 * before the `optimizer.step()` of train/train_*.py (the HF Trainer's max_grad_norm); they read the Adam job tables above: numel is
 * column 4 of the static rows, the gradient pointer column 0 of the per-step rows, a job with a null gradient contributes exact zeros
 * (it owns no partial: the sums are those of the table without that row).
 *
 * aptai_grad_sqnorm_multi, two launches on the stream: (1) one block per 4096-element chunk (the chunking of aptai_adam_multi) sums
 * the squares in fp32 in a fixed order and stores one partial at partials_dev[chunks of the jobs before it + chunk index];
 * partials_dev: room for fp32 [sum over jobs of ceil(n / 4096)].  (2) ONE block adds the partials in double - thread t takes t, t + 256, ...
 * in index order, then a fixed tree - takes the root in double and writes result_dev: fp32 [3] = {total_norm,
 * coef = min(1, max_norm / (total_norm + 1e-6)) evaluated in double and rounded once, number of gradient elements}.  NaN propagates;
 * total_norm = inf gives coef 0; max_norm = inf gives coef 1 (measure only).  No atomics: the summation order is a function of the
 * two tables, the same gradients give the same bits.  One table may span several parameter groups (one norm over all of them). */
int aptai_grad_sqnorm_multi(const int64_t* table_dev, const int64_t* dyn_dev, int64_t njobs, int64_t max_n, float* partials_dev,
                            float* result_dev, double max_norm, void* stream);
/* aptai_adam_multi on the gradient g * (*grad_scale_dev) (one rounded fp32 multiply, then the same update: weight decay is added to the
 * scaled gradient, as torch does after clip_grad_norm_).  The coefficient is read from device memory - result_dev + 1 of the call
 * above - so nothing is read back; the gradients themselves are NOT modified. */
int aptai_adam_multi_scaled(const int64_t* table_dev, const int64_t* dyn_dev, int64_t njobs, int64_t max_n, float lr, float beta1,
                            float beta2, float eps, float weight_decay, const float* grad_scale_dev, void* stream);
/* g *= *scale_dev in place for every job with a gradient (the in-place half of clip_grad_norm_, for a user's own loop): the same
 * single rounded multiply as aptai_adam_multi_scaled, so scale-then-step equals the fused step bit for bit. */
int aptai_scale_multi(const int64_t* table_dev, const int64_t* dyn_dev, int64_t njobs, int64_t max_n, const float* scale_dev,
                      void* stream);
/* Gradient accumulation over a window of N micro-batches (the HF Trainer's gradient_accumulation_steps), one launch per micro-step
 * over the Adam job table above (only n, column 4, is read).  acc_dev: device int64 [njobs] = one fp32 accumulator of n elements per
 * job; dyn_dev: device int64 [njobs][2] = {grad or 0 (no gradient in this micro-step), mode}:
 *   mode 0  the job has had no contribution in this window: its accumulator is neither read nor written;
 *   mode 1  first contribution of the window: acc = grad (an overwrite - there is no zeroing pass; grad must not be 0);
 *   mode 2  contributed before: acc = acc + grad, or untouched when grad is 0.
 * scale != 1 closes the window: every job of mode 1 or 2 is then multiplied by it, also one without a gradient in this call.
 * Arithmetic contract: one rounded fp32 add (__fadd_rn) per element per micro-step, in micro-step order, and one rounded fp32 multiply
 * (__fmul_rn) by scale = (float)(1.0 / k) at the close - the bits of ((g1 + g2) + ... + gk) * scale evaluated in fp32 in that order;
 * no division, no atomics, no dependence on the launch geometry.  16-byte vector path when n % 4 == 0 and both pointers are 16-byte
 * aligned, scalar path otherwise.  Validates and launches only (no allocation, copy or synchronisation): it runs between graph
 * replays.  Moves 12 B per parameter (8 B on a first contribution); the Adam launch moves 28 B. */
int aptai_grad_accum_multi(const int64_t* table_dev, const int64_t* dyn_dev, const int64_t* acc_dev, int64_t njobs, int64_t max_n,
                           float scale, void* stream);
/* Exponential moving average of the weights, one launch behind the Adam launches of an update, over the Adam job table above (only
 * the parameter pointer, column 0, and n, column 4, are read; there is no per-step row, so a job without a gradient in this update
 * still averages).  ema_dev: device int64 [njobs] = one fp32 average of n elements per job.  Per element
 *   ema = __fadd_rn(ema, __fmul_rn(weight, __fsub_rn(p, ema)))
 * - three rounded fp32 operations, no fused multiply-add: the bits of e + w * (p - e) evaluated with separate fp32 operations.
 * weight = (float)(1 - decay of this update), in (0, 1] (NaN is refused).  The chunking of aptai_adam_multi, every load of a thread
 * before its first store, no atomics; 16-byte vector path when n % 4 == 0 and both pointers are 16-byte aligned, scalar path
 * otherwise.  Validates and launches only (no allocation, copy or synchronisation).  Moves 12 B per parameter. */
int aptai_ema_multi(const int64_t* table_dev, const int64_t* ema_dev, int64_t njobs, int64_t max_n, float weight, void* stream);
/* Exchanges every job's parameter and its average element for element (same tables, chunking and paths): evaluation on the averaged
 * weights without moving a pointer.  Two calls are the identity, bit for bit.  Moves 16 B per parameter. */
int aptai_swap_multi(const int64_t* table_dev, const int64_t* ema_dev, int64_t njobs, int64_t max_n, void* stream);
/* nn.Conv1d weight [N][C][Kw] (HF:260-266) -> [N][Kw*C] bf16, K index = kw*C + c (channels-last frames) */
int aptai_conv_weight_to_bf16(const float* src, void* dst, int64_t N, int64_t C, int64_t Kw, void* stream);
/* positional conv (HF:329-356): weight_norm(dim=2) w = g*v/||v||_(0,1) ; v [H][H/groups][Kw], gain [Kw];
 * w_fwd [groups][Cg][Kw*Cg] (forward), w_dgrad [groups][Cg][Kw*Cg] (flipped taps, in/out swapped; may be null);
 * norm_ws fp32 [257 * Kw]: the first Kw entries receive ||v|| per tap (needed by the weight-norm backward), the rest is
 * scratch for the two-stage reduction; Kw must divide 256. */
int aptai_posconv_weight(const float* v, const float* gain, float* norm_ws, void* w_fwd, void* w_dgrad, int64_t H,
                         int64_t groups, int64_t Kw, void* stream);
/* Backward of that weight-norm parametrisation: from dw_fwd fp32 [groups][Cg][Kw*Cg] (the weight gradient in the forward layout)
 * to dv [H][Cg][Kw] and dgain [Kw] (HF parametrizations.weight.original1 / original0).  workspace fp32 [(H + 1) * Kw]. */
int aptai_posconv_weight_bwd(const float* dw_fwd, const float* v, const float* gain, const float* norm, float* dv, float* dgain,
                             float* workspace, int64_t H, int64_t groups, int64_t Kw, void* stream);
/* The grouped convolution itself for 48 channels per group and 128 taps (wav2vec2-base), replacing the batched implicit GEMM:
 * out[b*Tp+t][grp*48+n] = residual + act(bias + sum_{kw,c} xg[grp][b][first_row + t + kw][c] * w[grp][n][kw*48+c]);
 * xg as produced by aptai_posconv_pack ([groups][B][pad+Tp+pad][48], gap rows zero), w = w_fwd (forward, first_row 0,
 * bias + GELU, out_pre = pre-activation) or w_dgrad (data gradient, first_row 1); Tp % 128 == 0. */
int aptai_posconv_gemm(const void* xg, int64_t first_row, const void* w, const float* bias, const void* residual, void* out,
                       void* out_pre, int64_t B, int64_t Tp, int64_t H, int64_t groups, int64_t Kw, int64_t pad, int gelu,
                       void* stream);
/* Weight gradient of the same convolution: dw[grp][co][kw*48+ci] (fp32, overwritten) = sum_f du_g[grp][pad + f][co] *
 * x_g[grp][f + kw][ci] over the frame axis of the packed copies (gap rows are zero), replacing the batched TN GEMM. */
int aptai_posconv_wgrad(const void* du_g, const void* x_g, float* dw, int64_t B, int64_t Tp, int64_t H, int64_t groups, int64_t Kw,
                        int64_t pad, void* stream);
/* SpecAugment time mask sampled on the device (HF:101-217 `_compute_mask_indices` as called at HF:1292-1304): mask_u8 [B][T]
 * (overwritten), frame_lens int32 [B] valid frames per utterance.  Same span-count rule and without-replacement span starts as
 * the reference; counter-hash random stream keyed by `seed` (and the device seed salt). */
int aptai_spec_augment_mask(const int32_t* frame_lens, void* mask_u8, int64_t B, int64_t T, float mask_prob, int64_t mask_length,
                            int64_t min_masks, uint64_t seed, void* stream);
/* x [B*Tp][H] bf16 -> group-major, zero-gapped xg [groups][B][pad+Tp+pad][Cg] (gap rows must be pre-zeroed once);
 * with u != null the packed value is x*gelu'(u) (backward of HF:362) and rowmajor_out also receives it. */
int aptai_posconv_pack(const void* x, const void* u, void* xg, void* rowmajor_out, int64_t B, int64_t Tp, int64_t H,
                       int64_t groups, int64_t pad, void* stream);

/* ------------------------------------------------------------------------------------------------ frame masking
 * In place on h [B*Tp][H] bf16: frames t >= min(lens[b], T) -> 0 (HF:678-681); frames with spec_mask[b][t] != 0
 * (uint8 [B][T], sampled on the host exactly like HF:101-217) -> masked_spec_embed (HF:1292-1295). */
int aptai_frame_mask_fwd(void* h, const int32_t* lens, const uint8_t* spec_mask, const float* embed, int64_t B, int64_t Tp,
                         int64_t T, int64_t H, void* stream);
int aptai_frame_mask_bwd(void* dy, const int32_t* lens, const uint8_t* spec_mask, float* dembed, void* workspace, int64_t B,
                         int64_t Tp, int64_t T, int64_t H, void* stream);
int64_t aptai_frame_mask_bwd_workspace_bytes(int64_t B, int64_t Tp, int64_t H);
/* The same pass with SpecAugment along the hidden axis (HF `_mask_hidden_states`, `mask_feature_prob`): feat_mask uint8 [B][H],
 * 4-byte aligned, null = none.  Forward, after the time fill: h[b][t][c] = 0 on every valid frame t where feat_mask[b][c] != 0, so
 * a masked channel is zero on time-masked frames too.  Backward: dy is zeroed on padding, on time-masked frames and on
 * feature-masked channels; dembed[c] sums dy over the valid, time-masked rows whose feat_mask[b][c] is 0 (fixed order, no
 * atomics; workspace as aptai_frame_mask_bwd_workspace_bytes).  A feature mask without a time mask is legal (embed / dembed
 * null); a spec_mask without embed, a null h or lens and H % 4 != 0 are refused before any launch.  One pass over h / dy. */
int aptai_frame_feature_mask_fwd(void* h, const int32_t* lens, const uint8_t* spec_mask, const float* embed,
                                 const uint8_t* feat_mask, int64_t B, int64_t Tp, int64_t T, int64_t H, void* stream);
int aptai_frame_feature_mask_bwd(void* dy, const int32_t* lens, const uint8_t* spec_mask, const uint8_t* feat_mask, float* dembed,
                                 void* workspace, int64_t B, int64_t Tp, int64_t T, int64_t H, void* stream);

/* out[n] (+)= sum_rows x[row][n]  — bias gradients */
int aptai_colsum_bf16(const void* x, int64_t ld, float* out, void* workspace, int64_t rows, int64_t N, int accumulate,
                      void* stream);
int64_t aptai_colsum_workspace_bytes(int64_t rows, int64_t N);

/* y = keep ? x/(1-p) : 0 with the counter mask of (seed, element index) — standalone nn.Dropout forward/backward */
int aptai_dropout_bf16(const void* x, void* y, int64_t n, float p, uint64_t seed, void* stream);
/* out = dy * gelu'(u) — backward of a standalone GELU (top of the conv stack, HF:267-272) */
int aptai_dgelu_bf16(const void* dy, const void* u, void* out, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------------ conv layer 0
 * Conv1d(1,512,k=10,s=5) on the raw waveform fused with GroupNorm+GELU (mode 0, HF:302-323) or
 * bias+LayerNorm+GELU (mode 1, HF:275-299).  audio fp32 [B][S]; out bf16 [B][T_alloc][512], frames >= T_real zeroed. */
int aptai_conv0_fwd(const float* audio, int64_t B, int64_t S, const float* weight, const float* bias, const float* gamma,
                    const float* beta, int mode, float eps, void* out, int64_t T_real, int64_t T_alloc, int64_t C,
                    int64_t Kw, int64_t stride, void* workspace, float* stats_out, void* stream);
int64_t aptai_conv0_workspace_bytes(int64_t B, int64_t T_real);
/* Batch-invariant form of aptai_conv0_fwd (inference; Wav2Vec2Model.batch_invariant): the same operands plus frame_lens0, int32 [B] on
 * the device, utterance b's OWN first-layer frame count (len_b - 10) / 5 + 1 >= 1.  The effective count of a row is
 * n_b = max(1, min(frame_lens0[b], T_real, bounds[0] of aptai_set_frame_bounds when one is bound to the stream)).
 *   mode 0: the GroupNorm moments run over frames t < n_b only and are divided by n_b; out[b][t] = 0 for n_b <= t < T_alloc;
 *           stats_out [B][2][512] as in aptai_conv0_fwd (aptai_conv0_fwd_f32 / _split, which read it, follow unchanged).
 *   mode 1: the arithmetic of aptai_conv0_fwd, zeros for n_b <= t < T_alloc.
 * Row b - its valid frames and its stats_out row - is bit for bit what the utterance gets from this entry at B = 1, S = len_b: the moment
 * chunks (1024 frames) and a thread's frames within a chunk follow the frame index alone, the chunks of a row are summed in ascending
 * order and those wholly beyond n_b are neither computed nor read.  Frames are masked by selection: no sample at or beyond
 * 5 (n_b - 1) + 10 <= len_b reaches a result, whatever it holds (NaN included).  Both forms of the group-mode write pass are covered
 * (APTAI_CONV0_MFMA=1, the default, and 0).  Runs on `stream`, never synchronises, no atomics, capturable; workspace as
 * aptai_conv0_workspace_bytes(B, T_real).  The backward entries below do not know this form (inference only). */
int aptai_conv0_fwd_lens(const float* audio, int64_t B, int64_t S, const float* weight, const float* bias, const float* gamma,
                         const float* beta, int mode, float eps, void* out, int64_t T_real, int64_t T_alloc, int64_t C,
                         int64_t Kw, int64_t stride, void* workspace, float* stats_out, const int32_t* frame_lens0, void* stream);
/* backward of the same fused layer: recomputes the conv from the waveform, folds GELU' and the GroupNorm / LayerNorm
 * backward, and reduces dweight [512][10] (+ dbias, dgamma, dbeta) deterministically.  dy bf16 [B][T_alloc][512];
 * fwd_stats fp32 [B][2][512] = (mean, rstd) written by the forward (`stats_out`), group mode only. */
int aptai_conv0_bwd(const float* audio, int64_t B, int64_t S, const float* weight, const float* bias, const float* gamma,
                    const float* beta, int mode, float eps, const void* dy, int64_t T_real, int64_t T_alloc,
                    const float* fwd_stats, float* dweight, float* dbias, float* dgamma, float* dbeta, void* workspace,
                    void* stream);
int64_t aptai_conv0_bwd_workspace_bytes(int64_t B, int64_t T_real);
/* gradient w.r.t. the waveform of the same fused layer: du as in aptai_conv0_bwd (group mode: the same statistics pass), then
 * daudio[b][s] = sum over the frames t in {s/5 - 1, s/5} below T_real of sum_c W[c][s - 5 t] du[b][t][c].  daudio fp32 [B][S]: every
 * sample written (0 where no window reaches); dy rows >= T_real are not read by the data passes; deterministic (no atomics). */
int aptai_conv0_bwd_data(const float* audio, int64_t B, int64_t S, const float* weight, const float* bias, const float* gamma,
                         const float* beta, int mode, float eps, const void* dy, int64_t T_real, int64_t T_alloc,
                         const float* fwd_stats, float* daudio, void* workspace, void* stream);
int64_t aptai_conv0_bwd_data_workspace_bytes(int64_t B, int64_t T_real);

/* ------------------------------------------------------------------------------------------------ APTAI heads
 * a_tv = tanh(dropout(h)), a_ph = leaky_relu(dropout(h)) — the activations in front of the two head Linears
 * (models/aptai.py:43-55); the Linears themselves run on aptai_gemm_bf16 with N padded to 64. */
int aptai_head_act_fwd(const void* h, void* a_tv, void* a_ph, int64_t n, float p_tv, float p_ph, uint64_t seed, void* stream);
int aptai_head_act_bwd(const void* h, const void* d_tv, const void* d_ph, void* dh, int64_t n, float p_tv, float p_ph,
                       uint64_t seed, void* stream);
/* LowPassFilterLayer (models/modules.py:46-61): 51-tap 'same' FIR along time, fp64 accumulate, per channel.
 * x fp32 rows (b*rows_per_b_in + t) stride ldx; y fp32 or bf16 rows (b*rows_per_b_out + t) stride ldy; frames in
 * [T, T_out) and channels in [C, C_out) of y are zero-filled.  Symmetric taps: the same call is its own backward. */
int aptai_lowpass_fir(const float* x, int64_t ldx, int64_t rows_per_b_in, const double* taps, int64_t ntaps, void* y,
                      int64_t ldy, int64_t rows_per_b_out, int out_bf16, int64_t B, int64_t T, int64_t T_out, int64_t C,
                      int64_t C_out, void* stream);
/* Batch-invariant form: frame_lens int32 [B] on the device.  For row b the zero padding starts at
 * n_b = max(1, min(frame_lens[b], T, bounds[1] of aptai_set_frame_bounds when bound)): taps outside [0, n_b) weigh 0 and frames
 * n_b <= t < T_out are written as 0.  Tap order and the fp64 accumulate are those of aptai_lowpass_fir, so a row equals, bit for bit,
 * aptai_lowpass_fir on that utterance alone at T = n_b.  Same stream / no-sync / no-atomics / capture properties. */
int aptai_lowpass_fir_lens(const float* x, int64_t ldx, int64_t rows_per_b_in, const double* taps, int64_t ntaps, void* y,
                           int64_t ldy, int64_t rows_per_b_out, int out_bf16, int64_t B, int64_t T, int64_t T_out, int64_t C,
                           int64_t C_out, const int32_t* frame_lens, void* stream);
/* loss = w_mse * MSE(tv_pred[mask], tv_tgt[mask]) + w_ce * CE(logits[phn!=0], phn) and argmax (models/aptai.py:89-106;
 * models/force_aptai.py:137-141 with w_ce = 0).  scalars fp32[5] = loss, mse, ce, #valid tv elements, #valid frames. */
int aptai_aptai_loss_fwd(const float* tv_pred, const float* tv_tgt, const float* logits, int64_t ldl, int64_t rows_per_b,
                         const int64_t* phn_tgt, int64_t B, int64_t T, int64_t n_tv, int64_t n_phn, float w_mse, float w_ce,
                         float* scalars, int64_t* pred, void* workspace, void* stream);
int aptai_aptai_loss_bwd(const float* tv_pred, const float* tv_tgt, const float* logits, int64_t ldl, int64_t rows_per_b,
                         const int64_t* phn_tgt, int64_t B, int64_t T, int64_t n_tv, int64_t n_phn, float w_mse, float w_ce,
                         const float* scalars, const float* grad_out, float* d_tv, void* d_logits_bf16, int64_t ldd,
                         void* stream);
int64_t aptai_aptai_loss_workspace_bytes(void);

/* ------------------------------------------------------------------------------------------------ MX block-scaled FP8 GEMM
 * BASELINE configs[4] ("fp8 MFMA weights"): the frozen, inference-only encoder of Force_APTAI with OCP MXFP8 operands - E4M3
 * elements, one E8M0 scale per 32 consecutive k - on v_mfma_scale_f32_32x32x64_f8f6f4 (twice the bf16 MFMA rate on gfx950; no
 * reference counterpart: the reference is fp32).  aptai_mx_quantize_bf16: x bf16 [rows][K] -> q (1 byte / element,
 * row stride ldq) + scales (1 byte per 32 k, row stride lds); scale = 2^(floor(log2 amax) - 8), elements round-to-nearest-even,
 * saturated to +-448.  aptai_gemm_mxfp8: C bf16 [M][N] = dequant(A) . dequant(B)^T + bias, optional GELU, + residual;
 * replaces nn.Linear of the encoder layers (HF:495-498,546,556-572) when the model is switched to "mxfp8" inference. */
int aptai_mx_quantize_bf16(const void* x, int64_t ldx, void* q, int64_t ldq, void* scales, int64_t lds, int64_t rows, int64_t K,
                           void* stream);
int aptai_gemm_mxfp8(const void* A, const void* A_scales, int64_t lda, int64_t ldas, const void* B, const void* B_scales, int64_t ldb,
                     int64_t ldbs, void* C, int64_t ldc, const float* bias, int gelu, const void* residual, int64_t ldr, int64_t M,
                     int64_t N, int64_t K, void* stream);
/* The same product with an MXFP8 RESULT (elements Cq [M][ldcq], scales C_scales [M][ldcs], N % 32 == 0): bit-identical to aptai_gemm_mxfp8
 * followed by aptai_mx_quantize_bf16 of its bf16 output, without that tensor's trip through HBM - the FFN1 -> FFN2 hand-over of the
 * encoder layer (HF:556-572: intermediate_dense + GELU feeding output_dense). */
/* nn.LayerNorm (HF:500,556 of the pre-LN layer) whose result leaves as MXFP8 (q [rows][ldq], scales [rows][lds], one per 32 columns) and,
 * if y_bf16 is not null, as bf16 too: bit-identical to aptai_layernorm_fwd followed by aptai_mx_quantize_bf16. */
int aptai_layernorm_fwd_mx(const void* x, const float* gamma, const float* beta, void* y_bf16, void* q, int64_t ldq, void* scales,
                           int64_t lds, int64_t rows, int64_t cols, float eps, void* stream);
int aptai_gemm_mxfp8_mxout(const void* A, const void* A_scales, int64_t lda, int64_t ldas, const void* B, const void* B_scales, int64_t ldb,
                           int64_t ldbs, void* Cq, int64_t ldcq, void* C_scales, int64_t ldcs, const float* bias, int gelu, int64_t M,
                           int64_t N, int64_t K, void* stream);

/* ------------------------------------------------------------------------------------------------ CTC
 * log_softmax + CTC negative log-likelihood (alpha recursion) and its gradient w.r.t. the LOGITS (beta recursion),
 * replacing nn.functional.log_softmax + F.ctc_loss at models/w2v2_pr.py:59,73-81 and the per-sample nn.CTCLoss loop
 * of ForwardSumLoss (models/modules.py:99-116; vocab_sizes[b] = N_b + 1 classes, targets 1..N_b).
 * logits fp32 rows (b*rows_per_b + t) stride ldl; targets int32 [B][ldt] (any padding beyond target_lens[b]);
 * reduction 0 none / 1 mean (mean_b nll_b / max(len_b,1)) / 2 sum; nll fp32 [B]; loss fp32 scalar;
 * log_probs_out fp32 (T,B,V) or null; workspace (aptai_ctc_workspace_bytes) holds alpha | beta | per-state log-probs and is
 * handed unchanged to aptai_ctc_bwd.  want_beta != 0 runs the beta recursion beside the alpha recursion in the same launch
 * (both are sequential over T and independent of each other): the backward is then one parallel pass. */
int aptai_ctc_fwd(const float* logits, int64_t ldl, int64_t rows_per_b, const int32_t* targets, int64_t ldt,
                  const int32_t* input_lens, const int32_t* target_lens, const int32_t* vocab_sizes, int64_t B, int64_t T,
                  int64_t V, int blank, int reduction, int zero_infinity, float* log_probs_out, float* workspace, float* nll,
                  float* loss, int want_beta, void* stream);
/* dlogits rows (b*rows_per_b + t) stride ldd (V <= ldd <= 256), bf16 or fp32, zero outside t < input_lens[b] and v < V;
 * gradient = grad_out[0] (device scalar, may be null = 1) * extra_scale * d loss / d logits.  beta_ready = the forward call
 * was made with want_beta (otherwise the beta recursion runs here first). */
int aptai_ctc_bwd(const float* logits, int64_t ldl, int64_t rows_per_b, const int32_t* targets, int64_t ldt,
                  const int32_t* input_lens, const int32_t* target_lens, const int32_t* vocab_sizes, int64_t B, int64_t T,
                  int64_t V, int blank, int reduction, int zero_infinity, const float* workspace, const float* nll,
                  const float* grad_out, float extra_scale, void* dlogits, int64_t ldd, int out_bf16, int beta_ready, void* stream);
int64_t aptai_ctc_workspace_bytes(int64_t B, int64_t T, int64_t ldt);
/* Forced alignment of a KNOWN transcript: the best (Viterbi) path through the lattice aptai_ctc_fwd sums over.  Operands and
 * conventions of aptai_ctc_fwd (logits fp32 rows (b*rows_per_b + t) stride ldl; targets int32 [B][ldt]; input_lens, target_lens,
 * optional vocab_sizes; V <= 256; at most 255 labels; caller-owned workspace of aptai_ctc_viterbi_workspace_bytes, 16-byte
 * aligned; the passed stream; no synchronisation, no atomics, same inputs -> same bits), plus `topology`:
 *   0 = CTC: states blank, l1, blank, ..., lL, blank; transitions stay, +1, and +2 where the two labels differ;
 *   1 = monotonic, no blank: states l1 .. lL; transitions stay and +1; the path starts in l1 and ends in lL, so every label
 *       owns at least one frame (`blank` is ignored).
 * The path does not depend on the per-frame normaliser, so the recursion runs on the RAW logits of the extended states:
 * new[s] = best + x_t[ext_s], one fp32 addition per state and frame, first frame new[s] = x_0[ext_s] for the start states.
 * TIE RULE: the current state (stay) is the incumbent; the s-1 predecessor replaces it only if strictly greater; then the s-2
 * predecessor replaces that only if strictly greater.  The final state is the last one unless the one before it is strictly
 * greater (topology 1: always the last).  With that frame_token is a pure function of the fp32 inputs
 * (aptai_amd/hostlogic.py ctc_forced_align restates it in numpy).
 * Outputs: frame_token int32 [B][T]: transcript position 0..L-1 of each frame, -1 = blank frame, -2 = frame at or beyond
 * input_lens[b] and every frame of an utterance without a feasible path.  spans int32 [B][ldt][2]: first and one-past-last frame
 * of each position, -1, -1 = none.  score fp32 [B]: log-probability of the path under the per-frame log-softmax over the
 * utterance's classes (a sum over frames in a fixed order); -inf when no path exists (T_b too short, a label outside the
 * vocabulary, T_b == 0 with L > 0) - a result, not an error status; 0 for T_b == 0 and L == 0.  token_score fp32 [B][ldt] (may be
 * null): mean log-probability of the label over the frames of its span, -inf where the position has no span. */
int aptai_ctc_viterbi(const float* logits, int64_t ldl, int64_t rows_per_b, const int32_t* targets, int64_t ldt,
                      const int32_t* input_lens, const int32_t* target_lens, const int32_t* vocab_sizes, int64_t B, int64_t T,
                      int64_t V, int blank, int topology, void* workspace, int32_t* frame_token, int32_t* spans, float* score,
                      float* token_score, void* stream);
int64_t aptai_ctc_viterbi_workspace_bytes(int64_t B, int64_t T, int64_t ldt);
/* aptai_ctc_viterbi for a WIDE lattice: a long recording against its whole transcript (the stitched logits of the long-form
 * helpers, one block of rows per recording).  Operands, outputs, fill values and TIE RULE are exactly those of aptai_ctc_viterbi
 * with topology 0, so frame_token is the same pure function of the fp32 inputs (hostlogic.ctc_forced_align) and for ldt <= 255
 * all four outputs equal aptai_ctc_viterbi's bit for bit.  Limits: 1 <= ldt <= APTAI_CTC_VITERBI_WIDE_MAX_LABELS (at most
 * 2 * 8191 + 1 = 16383 states); V <= 256; topology must be 0 (1 is refused: the monotonic lattice stays with aptai_ctc_viterbi).
 * One workgroup per recording walks the frames with one barrier per frame; there is no per-state emission matrix.
 * Workspace (aptai_ctc_viterbi_wide_workspace_bytes, 16-byte aligned, caller-owned):
 *   lz fp32 [B*T] (rounded up to 16 bytes) | backpointers [B][T][ceil((2 ldt + 1) / 16)] 32-bit words, two bits per state
 *   (0 stay, 1 from s-1, 2 from s-2), state s in bits [2 (s % 16), 2 (s % 16) + 2) of word s / 16.
 * About 30 MB for 15 000 frames and 4 000 labels.  No synchronisation, no atomics, same inputs -> same bits. */
#define APTAI_CTC_VITERBI_WIDE_MAX_LABELS 8191
int aptai_ctc_viterbi_wide(const float* logits, int64_t ldl, int64_t rows_per_b, const int32_t* targets, int64_t ldt,
                           const int32_t* input_lens, const int32_t* target_lens, const int32_t* vocab_sizes, int64_t B, int64_t T,
                           int64_t V, int blank, int topology, void* workspace, int32_t* frame_token, int32_t* spans, float* score,
                           float* token_score, void* stream);
int64_t aptai_ctc_viterbi_wide_workspace_bytes(int64_t B, int64_t T, int64_t ldt);
/* Best-path CTC decode on the device (stand-in for the torchaudio beam decoder the reference calls at models/w2v2_pr.py:143-159,
 * which is absent here: parity unpinned).  Row b is exactly hostlogic.ctc_bracketed_best_path(logits[b], T_b, blank, sil)
 * (aptai_amd/hostlogic.py, the oracle of the tests): frame argmax (first maximum) over the first T_b = clamp(input_lens[b], 0, T)
 * frames (input_lens null: all T; frames at or past T_b are not read), repeats collapsed, blank dropped.  sil < 0: no framing, the
 * timestep of a kept label is its frame t.  sil >= 0 (sil < V, sil != blank): the row is framed as the beam search below frames
 * it - sil at timestep 0, frame t at timestep t + 1, sil at timestep T_b + 1, repeats collapsed over that T_b + 2 long row, so a
 * silence on the first or last own frame merges with the framing one and a blank in between keeps both; T_b == 0 gives [sil] at 0.
 * ids_out and timesteps_out (may be null) int32 [B][max_n] hold the first max_n entries, zero-padded (the aligner's phoneme slots,
 * models/force_aptai.py:109-115); n_out int32 [B] = full decoded length, which the caller compares with max_n
 * (models/force_aptai.py:111).  One wave per utterance, no atomics: same inputs -> same bits.  Non-finite logits are not supported. */
int aptai_ctc_greedy_decode(const float* logits, int64_t ldl, int64_t rows_per_b, const int32_t* input_lens, int64_t B, int64_t T,
                            int64_t V, int blank, int sil, int32_t* ids_out, int32_t* timesteps_out, int64_t max_n, int32_t* n_out,
                            void* stream);
/* Lexicon-free CTC beam search without a language model, on the device: the decoder the reference calls through torchaudio
 * (models/w2v2_pr.py:143-159, flashlight's LexiconFreeDecoder with a zero LM) as its published sources state it, with n-best
 * lists, true prefix scores (log_add) and per-token timesteps.  aptai_amd/hostlogic.py ctc_beam_search restates the same search
 * in Python and is what the tests compare against; torchaudio itself is not available to this project: parity with it is unpinned.
 * logits fp32 rows (b*rows_per_b + t) stride ldl (the layout of aptai_ctc_greedy_decode); input_lens int32 [B] or null (= all T
 * frames of every row); V <= 256; blank != sil, both < V; beam_size 1..APTAI_BEAM_MAX; beam_size_token 0 = all V tokens, else the
 * k best tokens of each frame (ties to the lower id); beam_threshold >= 0; nbest 1..beam_size; caller-owned workspace of
 * aptai_ctc_beam_search_workspace_bytes, 16-byte aligned; the passed stream; no synchronisation.
 * A hypothesis is (token history, last token, last-was-blank) and starts as (empty, sil, no) with score 0.  Per frame t every
 * hypothesis is extended by every token n of the token beam: sc = (score + (double)x[t][n]) + (n == sil ? sil_score : 0) in fp64,
 * in that order.  A non-blank n that differs from the last token, or follows a blank, extends the history; a blank keeps it and
 * sets the flag; a repeat keeps it.  Candidates below (frame maximum - beam_threshold) are dropped; candidates of equal state
 * merge, the best one's back-pointer survives; its score stays (log_add 0) or the scores are folded with logaddexp in descending
 * order starting from the best (log_add 1); the beam_size best merged candidates survive.  Histories are equal when their token
 * sequences are, for the whole utterance, also when a history left the beam and is reached again.  After the last frame every
 * hypothesis takes the closing silence, which makes its state (history, sil, no): equal histories merge, floor and cut are applied
 * once more and the nbest best are read out: the T_b + 2 token row (opening silence, one token per frame, closing silence) has its
 * repeats collapsed and its blanks dropped, the row positions kept are the timesteps (a frame t appears as t + 1).  T_b == 0 gives
 * the single hypothesis [sil] at timestep 0 with score 0.
 * TIE RULE: of two candidates with exactly equal scores the one from the lower beam slot (the better parent) comes first, then
 * the lower token id, in the merge (whose back-pointer survives) as in the selection.  No atomics: same inputs -> same bits.
 * Outputs: tokens, timesteps int32 [B][nbest][max_n], zero-padded; n_tok int32 [B][nbest] = full length (what exceeds max_n is
 * cut, as in aptai_ctc_greedy_decode), 0 for a rank without hypothesis; score fp64 [B][nbest], -inf for a rank without hypothesis;
 * n_hyp int32 [B] = hypotheses returned for the row.  Non-finite logits are not supported (a NaN never wins a comparison). */
#define APTAI_BEAM_MAX 32
#define APTAI_BEAM_MAX_V 256
int aptai_ctc_beam_search(const float* logits, int64_t ldl, int64_t rows_per_b, const int32_t* input_lens, int64_t B, int64_t T,
                          int64_t V, int blank, int sil, int beam_size, int beam_size_token, double beam_threshold, int log_add,
                          double sil_score, int nbest, int64_t max_n, void* workspace, int32_t* tokens, int32_t* timesteps,
                          int32_t* n_tok, double* score, int32_t* n_hyp, void* stream);
/* 0 for arguments outside the limits above */
int64_t aptai_ctc_beam_search_workspace_bytes(int64_t B, int64_t T, int64_t beam_size, int64_t nbest);
/* The same search with a token-level n-gram language model fused in (flashlight's lm= / lm_weight= of the LexiconFreeDecoder; the
 * reference passes lm=None, torchaudio and KenLM are not available to this project: parity with them is unpinned).  Arguments,
 * workspace (aptai_ctc_beam_search_workspace_bytes), outputs, tie rule and determinism are those of aptai_ctc_beam_search; the
 * oracle is the same hostlogic.ctc_beam_search with lm=.  The model arrives as a dense automaton over lm_states contexts
 * (aptai_amd/ngram.py NGramLM.device_tables), ALREADY MULTIPLIED by the LM weight on the host, no multiply happens on the device:
 *   lm_w      fp64  [lm_states][V]  weight * ln P(n | state)          lm_next  int32 [lm_states][V]  state after token n
 *   lm_wfinal fp64  [lm_states]     weight * ln P(</s> | state)       lm_start the state of the empty history
 * A candidate that EXTENDS its history (a non-blank n that differs from the last token or follows a blank) scores
 * sc = ((score + (double)x[t][n]) + (n == sil ? sil_score : 0)) + lm_w[state(history)][n], fp64 adds in that order; blanks and
 * repeats take no term.  The new history's state is lm_next[state(parent history)][n]; a history has one state for the whole
 * utterance, so "equal token sequences merge" is unchanged.  The frame floor is (maximum over ALL candidates, LM term included)
 * - beam_threshold.  The closing silence adds lm_wfinal[state(history)] before its floor, whose maximum is over all hypotheses.
 * T_b == 0 gives [sil] at timestep 0 with score 0 + lm_wfinal[lm_start].  The silence token is an ordinary LM word; the blank
 * column of the tables is never read.  An all-zero model gives the bits of aptai_ctc_beam_search.
 * Refused with a message, launching nothing: null tables, lm_states < 1, lm_start outside [0, lm_states), lm_states * V > 2^24.
 * NOT checked on the device: entries of lm_next outside [0, lm_states) and non-finite scores (NGramLM checks both when it builds
 * its tables). */
int aptai_ctc_beam_search_lm(const float* logits, int64_t ldl, int64_t rows_per_b, const int32_t* input_lens, int64_t B, int64_t T,
                             int64_t V, int blank, int sil, int beam_size, int beam_size_token, double beam_threshold, int log_add,
                             double sil_score, int nbest, int64_t max_n, void* workspace, int32_t* tokens, int32_t* timesteps,
                             int32_t* n_tok, double* score, int32_t* n_hyp, const double* lm_w, const int32_t* lm_next,
                             const double* lm_wfinal, int64_t lm_states, int lm_start, void* stream);

/* ------------------------------------------------------------------------------------------------ Force_APTAI heads (fp32)
 * Small layers behind the frozen encoder of models/force_aptai.py:108-161.  fp32 because they feed an argmax whose
 * indices must match the reference. */
/* C[m][n] (+)= alpha*sum_k A(m,k)*B(k,n) + bias[n];  A(m,k)=A[m*sam+k*sak] (fp32, or bf16 when a_bf16),
 * B(k,n)=B[k*sbk+n*sbn]; `batch` problems at element strides bsa/bsb/bsc.  Replaces nn.Linear (force_aptai.py:122,
 * modules.py:140-141,195-201) and torch.bmm (modules.py:144,149). */
/* Runs on the f32-input matrix instruction (v_mfma_f32_32x32x2_f32): exact fp32 products and accumulation.  split_k > 1 cuts K
 * into slabs (partials in `workspace`, aptai_sgemm_workspace_bytes, summed in slab order: deterministic) for gradient-shaped
 * problems whose M x N alone cannot fill the chip. */
int aptai_sgemm_f32(const void* A, int a_bf16, int64_t sam, int64_t sak, const float* B, int64_t sbk, int64_t sbn, float* C,
                    int64_t ldc, const float* bias, float alpha, int accumulate, int64_t M, int64_t N, int64_t K, int64_t batch,
                    int64_t bsa, int64_t bsb, int64_t bsc, int64_t split_k, float* workspace, void* stream);
int64_t aptai_sgemm_workspace_bytes(int64_t M, int64_t N, int64_t batch, int64_t split_k);
/* nn.Embedding(padding_idx=0) + PositionalEncoding (force_aptai.py:118-119, modules.py:217-235): out[r] = emb[ids[r]] + pe[r % N] */
int aptai_embed_pe_fwd(const int32_t* ids, const float* emb, const float* pe, float* out, int64_t rows, int64_t N, int64_t D,
                       float dropout_p, uint64_t seed, void* stream);
int aptai_embed_bwd(const int32_t* ids, const float* dout, float* demb_zeroed, int64_t rows, int64_t D, float dropout_p,
                    uint64_t seed, void* stream);
/* CrossAttention softmax + the log-softmax alignment of force_aptai.py:128-130 and its argmax read-out (:148):
 * energy = raw + mask, att = softmax(energy), att_log = log_softmax(energy + mask), mask = -1000 where phn_ids == 0;
 * align int64 [B][T] = argmax_n att_log (first maximum), bit-exact integer output.  fs_rows (optional, [B*T][64]): the rows
 * ForwardSumLoss feeds its CTC (models/modules.py:90-98) - blank log-prob -1 | att_log | zeros.  bwd: d_attlog rows have
 * stride ld_dattlog (0 = N), so the CTC gradient of those 64-float rows is read in place (pointer + 1). */
int aptai_xattn_softmax_fwd(const float* raw, const int32_t* phn_ids, float* energy, float* att, float* att_log, int64_t* align,
                            float* fs_rows, int64_t B, int64_t T, int64_t N, void* stream);
int aptai_xattn_softmax_bwd(const float* att, const float* att_log, const float* d_att, const float* d_attlog, int64_t ld_dattlog,
                            float* d_raw, int64_t rows, int64_t N, void* stream);
/* The same pair for 64 <= N <= 255 phoneme slots (Force_APTAI(max_phn_seq_len=...)): a lane holds slots l, l + 64, l + 128, l + 192.
 * fs_rows has pitch ld_fs = round_up(N + 1, 64) floats (64 .. 256) with the same content, -1 | att_log[0..N) | zeros.  Among equal
 * maxima align is the lowest slot index.  A transcript short enough for the pair above gets that pair's bits in its own columns. */
int aptai_xattn_softmax_fwd_wide(const float* raw, const int32_t* phn_ids, float* energy, float* att, float* att_log, int64_t* align,
                                 float* fs_rows, int64_t ld_fs, int64_t B, int64_t T, int64_t N, void* stream);
int aptai_xattn_softmax_bwd_wide(const float* att, const float* att_log, const float* d_att, const float* d_attlog,
                                 int64_t ld_dattlog, float* d_raw, int64_t rows, int64_t N, void* stream);
int aptai_layernorm_f32_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, int64_t rows,
                            int64_t cols, float eps, void* stream);
int aptai_layernorm_f32_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma, float* dx,
                            float* dgamma, float* dbeta, float* workspace, int64_t rows, int64_t cols, void* stream);
int64_t aptai_layernorm_f32_bwd_workspace_bytes(int64_t cols);
/* nn.LSTM(256,256,bidirectional) over packed sequences (modules.py:195,204-206): xproj [B*Tp][2][1024] = x W_ih^T + b_ih + b_hh,
 * whh [2][1024][256] (weight_hh_l0, weight_hh_l0_reverse as stored), lens int32 [B]; hout [B*Tp][512] (zeros beyond lens);
 * gates (post-activation i,f,g,o) [B*Tp][2][1024] and cstate [B*Tp][2][256] are saved for the backward (both null in
 * inference).  GATE LAYOUT of xproj, gates and dgates (round 4): column dir * 1024 + unit * 4 + gate - gate-INTERLEAVED, i.e. the rows of
 * W_ih and of the bias sum permuted from torch's gate-major order by the caller (row unit * 4 + gate of the operand = row gate * 256 + unit
 * of weight_ih_l0); whh keeps torch's order.  The *_serial cross-check kernels keep the gate-major layout.  16 cooperating workgroups per (16 utterances, direction) keep W_hh in registers and exchange h through
 * `workspace` (aptai_lstm_workspace_bytes; zero-initialised ONCE by the caller, its first 256 bytes are a status word that
 * turns non-zero if a bounded wait ever timed out).  bwd: dgates [B*Tp][2][1024] = gradients w.r.t. the gate pre-activations
 * (zeros beyond lens). */
int aptai_lstm_fwd(const float* xproj, const float* whh, const int32_t* lens, float* hout, float* gates, float* cstate,
                   void* workspace, int64_t B, int64_t Tp, int64_t T, int64_t hidden, void* stream);
int aptai_lstm_bwd(const float* dhout, const float* whh, const int32_t* lens, const float* gates, const float* cstate, float* dgates,
                   void* workspace, int64_t B, int64_t Tp, int64_t T, int64_t hidden, void* stream);
int64_t aptai_lstm_workspace_bytes(int64_t B);
/* the same recurrences, one block per (utterance, direction), W_hh streamed from L2 on every frame (whhT [2][256][1024] for the
 * forward): the on-device cross-check of the kernels above, not on the hot path */
int aptai_lstm_fwd_serial(const float* xproj, const float* whhT, const int32_t* lens, float* hout, float* gates, float* cstate,
                          int64_t B, int64_t Tp, int64_t T, int64_t hidden, void* stream);
int aptai_lstm_bwd_serial(const float* dhout, const float* whh, const int32_t* lens, const float* gates, const float* cstate,
                          float* dgates, int64_t B, int64_t Tp, int64_t T, int64_t hidden, void* stream);
/* pred_frame_phns (force_aptai.py:152-161): out[b][t] = phn_table[b][align[b][t]] for t < lens[b], else -1 (int64) */
int aptai_gather_alignment(const int32_t* phn_table, const int64_t* align, const int32_t* lens, int64_t* out, int64_t B, int64_t T,
                           int64_t N, void* stream);
int aptai_tanh_dropout_f32(const float* x, const float* y_or_null, const float* dy_or_null, float* out, int64_t n, float dropout_p,
                           uint64_t seed, void* stream);
int aptai_dropout_f32(const float* x, float* y, int64_t n, float dropout_p, uint64_t seed, void* stream);
/* out[n] = sum_r x[r*ld + n] (bias gradients of the fp32 heads), two deterministic stages through `workspace` */
int aptai_colsum_f32(const float* x, int64_t ld, float* out, float* workspace, int64_t rows, int64_t N, void* stream);
int64_t aptai_colsum_f32_workspace_bytes(int64_t N);

/* ------------------------------------------------------------------------------------------------ evaluation metrics
 * What validate()/test() of the reference's train_*.py compute on the host per utterance, on the device: raw pointers and
 * pitches, int32 length vectors on the device, caller-owned outputs, the passed stream, no synchronisation, no atomics (fixed
 * reduction order: lane-strided partials, a shuffle tree, then the waves in order; same inputs -> same bits).  Elements at or
 * beyond a length are never read into a result.  All of these are latency-bound: one block or one wave per utterance. */
/* tvs_metric_rmse / tvs_metric_ppc (utility.py:393-444).  gt, pred fp32: element (b, t, c) at (b*rows + t)*ld + c, each with its
 * own rows and pitch; lens int32 [B], clamped to [0, max_len]; C tracks.  rmse, pcc fp64 [B][C], all arithmetic fp64 on the
 * widened inputs.  rmse = sqrt(sum (x-y)^2 / T).  Pearson as scipy: means first, then centred sums, r = sxy / sqrt(sxx * syy)
 * clipped to [-1, 1]; NaN where a track is constant over its T frames (T == 1 included); T == 0 gives NaN in both. */
int aptai_eval_tv_scores(const float* gt, int64_t ldg, int64_t rows_g, const float* pred, int64_t ldp, int64_t rows_p,
                         const int32_t* lens, int64_t B, int64_t max_len, int64_t C, double* rmse, double* pcc, void* stream);
/* torch.eq(gt, pred).sum() of the loops and evaluate_overlap (utility.py:615-622): gt, pred int64 [B][ld]; counts int32 [B][2] =
 * {frames = lens[b] clamped to [0, max_len], frames with gt == pred}. */
int aptai_eval_frame_scores(const int64_t* gt, int64_t ldg, const int64_t* pred, int64_t ldp, const int32_t* lens, int64_t B,
                            int64_t max_len, int32_t* counts, void* stream);
/* get_stats (utility.py:588-612): y fp64 [B][ldy] with ny int32 [B], yhat fp64 [B][ldh] with nh; counts int32 [B][2] =
 * {precision_counter = #{j : min_i |y_i - yhat_j| <= tolerance}, recall_counter = #{i : min_j |y_i - yhat_j| <= tolerance}} with
 * numpy's fp64 subtraction, abs and compare, so the counts are exact.  ny == 0 or nh == 0 gives {0, 0}.  One block per
 * utterance, the other side staged through LDS in chunks. */
int aptai_eval_boundary_counts(const double* y, int64_t ldy, const int32_t* ny, const double* yhat, int64_t ldh, const int32_t* nh,
                               double tolerance, int64_t B, int32_t* counts, void* stream);
/* phn_frame_id2phn (utility.py:561-566): runs of equal labels collapsed.  x int64 [B][ld], lens int32 [B]; out int32 [B][ldo]
 * zero-padded, n_out int32 [B] = collapsed length (may exceed ldo: the caller checks; never when ldo >= ld). */
int aptai_eval_collapse_runs(const int64_t* x, int64_t ld, const int32_t* lens, int64_t B, int32_t* out, int64_t ldo, int32_t* n_out,
                             void* stream);
/* editdistance.eval (train/train_force_aptai.py:582, train/train_phoneme_recognizer.py:540): Levenshtein distance of B pairs.
 * a int32 [B][lda] with a_lens, b int32 [B][ldb] with b_lens (lengths clamped to the row length); dist int32 [B].  One wave per
 * pair; `a` lives in registers, 64 lanes x {1, 4, 8, 16, 32} rows picked from lda, so lda <= APTAI_EVAL_EDIT_MAX_LANE_SIDE (a
 * status names both row lengths otherwise; the distance is symmetric, so the caller puts the side that fits in `a`); b is
 * unbounded: b_len + 63 steps.  An empty side gives the other side's length. */
#define APTAI_EVAL_EDIT_MAX_LANE_SIDE 2048
int aptai_eval_edit_distance(const int32_t* a, int64_t lda, const int32_t* a_lens, const int32_t* b, int64_t ldb,
                             const int32_t* b_lens, int64_t B, int32_t* dist, void* stream);

/* ------------------------------------------------------------------------------------------------ audio front end
 * The step in front of the models that the reference runs on the host inside __getitem__ (data/dataset_commonphone.py:28-33,
 * data/dataset_hprc.py:68-70): resampling to 16 kHz, and the feature extractor's normalisation.  Caller-owned buffers, device
 * int64 offsets / lengths, the passed stream, no synchronisation, no atomics: equal inputs give equal bits. */
/* torchaudio.functional.resample (sinc_interp_hann) of B utterances in one launch.  src: all utterances back to back, float32
 * (src_is_int16 = 0) or int16 PCM (1; a sample counts as i / 32768 exactly), 16-byte aligned; offsets int64 [B + 1]: utterance b is
 * src[offsets[b] .. offsets[b+1]), nothing outside that range is read for it (it counts as 0.0).  taps fp32 [new][Kc] and first
 * int32 [new]: the compact filter bank of hostlogic.resample_taps for the reduced ratio orig -> new, `width` its half width:
 *     y[q new + p] = sum_{j < Kc} taps[p][j] x[q orig + first[p] + j - width]      (fp32 fused multiply-adds, j ascending, from 0)
 * a sequence that depends on nothing but the sample itself.  out fp32 [B][ld]: column c < ncols of row b is output sample
 * out_start[b] + c (out_start int64 [B] on the device, or null for 0), and exactly 0.0 at or beyond the utterance's
 * ceil(new len / orig) samples; columns ncols .. ld-1 are left alone.  orig == new copies (taps, first may be null).  A table of
 * more than APTAI_RESAMPLE_MAX_TABLE entries (new * Kc) is refused; one that fits LDS is staged there, a larger one is read
 * through L2. */
#define APTAI_RESAMPLE_MAX_TABLE (1 << 22)
int aptai_resample_batch(const void* src, int src_is_int16, const int64_t* offsets, int64_t B, const float* taps, const int32_t* first,
                         int64_t orig, int64_t new_, int64_t Kc, int64_t width, const int64_t* out_start, float* out, int64_t ld,
                         int64_t ncols, void* stream);
/* aptai_resample_batch with a ratio per row (speed perturbation: row b at speed f is the source taken as sampled at
 * round(rate f) and resampled to the target rate).  ratio int32 [B] on the device: row b runs at entry ratio[b] of `table`, int32
 * [n_ratios][8] on the device, n_ratios <= APTAI_RESAMPLE_MAX_RATIOS; an entry is {orig, new, Kc, width, taps_off, first_off, 0, 0}
 * and its bank is taps[taps_off .. taps_off + new Kc) / first[first_off .. first_off + new) of the concatenated fp32 / int32 arrays
 * (n_taps / n_first entries; an entry with orig == new copies and has no bank).  table_host and ratio_host are the same words in
 * host memory: the entry point checks them (every index inside the table, every bank inside the arrays) and takes the launch
 * geometry from them - the tile is the smallest one that aptai_resample_batch would pick for a ratio present in the batch.  Row b
 * has ceil(new len / orig) samples of ITS ratio and holds, bit for bit, what aptai_resample_batch writes for that utterance alone
 * with that bank: the sum is the same fma sequence whatever the tile, the neighbours, the crop, or whether a bank is staged in LDS
 * (decided per row: one that fits is, another is read through L2).  src, offsets, out_start, out, ld, ncols: as above. */
#define APTAI_RESAMPLE_MAX_RATIOS 8
int aptai_resample_batch_multi(const void* src, int src_is_int16, const int64_t* offsets, int64_t B, const float* taps, int64_t n_taps,
                               const int32_t* first, int64_t n_first, const int32_t* table, const int32_t* table_host, int64_t n_ratios,
                               const int32_t* ratio, const int32_t* ratio_host, const int64_t* out_start, float* out, int64_t ld,
                               int64_t ncols, void* stream);
/* The frame-level targets of a batch stretched with its audio, one launch: R_trk rows of fp64 tracks [R_trk][ld_in] and R_lab rows
 * of int64 frame labels [R_lab][ld_in]; row r (tracks first, then labels) goes from n_in[r] to n_out[r] frames (int64 on the
 * device, R_trk + R_lab entries, clamped to [0, T_in] / [0, T_out]).  Positions are numpy.linspace(0, n_in - 1, n_out):
 * p_i = i ((n_in - 1) / (n_out - 1)), the last one n_in - 1 exactly, 0 when n_out == 1.  Tracks: hostlogic.interpolate_signal
 * operation for operation in fp64 without contraction, out[i] = x[lo] + (x[hi] - x[lo]) w with lo = clip(floor(p), 0,
 * max(n_in - 2, 0)), w = p - lo, hi = min(lo + 1, n_in - 1); -100 where x[lo] == -100 or (w > 0 and x[hi] == -100); columns
 * n_out .. T_out-1 are -100.  Labels: out[i] = lab[min(floor(p_i + 0.5), n_in - 1)], padding 0.  n_in == n_out copies the row;
 * n_in == 0 gives a row of padding.  Equal inputs give the bits of hostlogic.warp_track / warp_frame_labels. */
int aptai_warp_targets(const double* tracks, int64_t R_trk, const int64_t* labels, int64_t R_lab, int64_t ld_in, int64_t T_in,
                       const int64_t* n_in, const int64_t* n_out, double* tracks_out, int64_t* labels_out, int64_t ld_out, int64_t T_out,
                       void* stream);
/* Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm in place on x fp32 [B][ld]: y = (x - mean) / sqrt(var + 1e-7) over the first
 * lens[b] samples of row b (lens int64 [B] on the device, clamped to [0, ncols]), population variance; the rest of the row is
 * not touched.  Statistics and the affine step in fp64 (sums of x - x[b][0], so a large offset does not cancel), summed in a
 * fixed order through `workspace` (aptai_wave_normalize_workspace_bytes), one rounding to fp32.  A row of length 0 is left as it
 * is; a constant row becomes zeros. */
int aptai_wave_normalize(float* x, int64_t ld, const int64_t* lens, int64_t B, int64_t ncols, void* workspace, void* stream);
int64_t aptai_wave_normalize_workspace_bytes(int64_t B, int64_t ncols);

/* ------------------------------------------------------------------------------------------------ long recordings
 * Overlapped-window inference over recordings longer than the clips the models were trained on (HF pipelines: chunk_length_s /
 * stride_length_s; the reference has no such path, models/aptai.py:125 runs the whole waveform through one forward).  The window
 * plan is hostlogic.long_form_plan: windows of window_frames encoder frames every hop_frames frames, K = 0 for a recording of
 * F <= window_frames frames and ceil((F - window_frames) / hop_frames) otherwise, windows 0 .. K.  Caller-owned buffers, device
 * int64 tables, the passed stream, no synchronisation, no atomics, no LDS: equal inputs give equal bits. */
/* The windows first .. first + rows - 1 of `table` cut out of src into the zero-padded batch the encoder takes, one launch.  src:
 * fp32, n_src elements, one or more recordings back to back.  table int64 [n_windows][3] on the device: {offset of the window's
 * recording in src, first sample of the window within the recording, sample count}.  out fp32 [rows][ld]: column c < S of row i
 * is src[offset + start + c] for c < count and exactly 0.0 beyond; columns S .. ld-1 are left alone.  lens_out int64 [rows]: the
 * counts (what the encoder takes as the rows' lengths).  Nothing outside [offset + start, offset + start + count) is read for a
 * window, so nothing past a recording's end when the table follows the plan; a count is cut to S and to what src holds, and an
 * entry with a negative field or a start outside src counts as empty: no table makes the kernel read outside src.  16-byte stores
 * when out is 16-byte aligned and ld % 4 == 0, scalar stores otherwise; first + rows <= n_windows, rows <= 65535. */
int aptai_window_gather(const float* src, int64_t n_src, const int64_t* table, int64_t n_windows, int64_t first, int64_t rows,
                        float* out, int64_t ld, int64_t S, int64_t* lens_out, void* stream);
/* Per-window results stitched into one row of frames per recording, one launch.  x: fp32 rows of pitch ldx, window w at rows
 * w rows_per_window .. (frame j of the window at row w rows_per_window + j), n_windows windows: the filtered trajectories
 * [W][T][n_tv] (ldx = n_tv, rows_per_window = T) and the padded head or CTC logits [W * Tp][Np] (ldx = Np, rows_per_window = Tp) as
 * they are.  rec int64 [n_rec][3] on the device: {first window of the recording in x, its frame count F, its first row in out};
 * its windows are consecutive in x.  Output frame t < F of a recording, channel c < C, with k = min(t / hop_frames, K) and
 * j = t - k hop_frames:
 *     j >= overlap = window_frames - hop_frames, or k == 0:   x1 = frame j of window k
 *     otherwise, x0 = frame j + hop_frames of window k - 1:   x0 where ramp[j] <= 0, x1 where ramp[j] >= 1, else
 *                                                             __fadd_rn(x0, __fmul_rn(ramp[j], __fsub_rn(x1, x0)))
 * - three rounded fp32 operations, no fused multiply-add (the rule of aptai_ema_multi).  ramp: fp32 [overlap] on the device
 * (hostlogic.long_form_ramp; may be null when no recording has a second window).  out fp32 [out_rows][ldo]: row rec[r][2] + t,
 * columns 0 .. C-1; columns C .. ldo-1 and rows no recording owns are left alone, every owned element is written exactly once.
 * argmax (optional) int64 [out_rows]: the index of the largest of the C stitched values of the frame, the lowest index on ties
 * (torch.argmax of a frame without ties; the rule of aptai_aptai_loss_fwd's phn_pred).  Non-finite inputs are not supported (a NaN
 * loses every comparison).  One wavefront per output frame, lanes over channels: 1 <= C <= 256.  window_frames / 2 <= hop_frames
 * <= window_frames (a frame is covered by one or two windows); max_frames >= every F (the grid) and rows_per_window >=
 * min(window_frames, max_frames); n_rec <= 65535.  A recording whose table entry points outside x or out (F > max_frames, a window
 * >= n_windows, a row >= out_rows) is skipped: no table makes the kernel write outside out. */
int aptai_stitch_windows(const float* x, int64_t ldx, int64_t rows_per_window, int64_t n_windows, const int64_t* rec, int64_t n_rec,
                         int64_t max_frames, int64_t window_frames, int64_t hop_frames, const float* ramp, int64_t C, float* out,
                         int64_t ldo, int64_t out_rows, int64_t* argmax, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* APTAI_HIP_H */
