/* rrt_hip.h -- C ABI of librrt_hip.so: the MI355X (gfx950) RRTEncoder forward path.
 *
 * The reference (DearCaat/RRT-MIL) has no FFI: its boundary for this path is the
 * Python class modules/rrt.py:133-202 `RRTEncoder(nn.Module)`.  These entry points
 * are what that class's forward binds to once its internals are replaced
 * (INTEGRATION.md shows the ctypes stub); each one cites the reference lines it
 * replaces.  Plain pointers and sizes only, no torch types.  All pointers are
 * DEVICE pointers (HIP) unless marked host; `stream` is a hipStream_t passed as
 * void*.  Nothing allocates: the caller owns a workspace sized by
 * rrt_encoder_workspace_size().  Every call is asynchronous on `stream`,
 * re-entrant and stateless.
 *
 * Return value: 0 = ok; <0 = RRT_E_* (unsupported/invalid, nothing launched);
 * >0 = hipError_t from a launch.
 */
#ifndef RRT_HIP_H
#define RRT_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RRT_ABI_VERSION 29
#define RRT_MAX_RMSA_LAYERS 8
#define RRT_MAX_CRMSA_K 8

enum {
  RRT_OK = 0,
  RRT_E_INVALID = -1,       /* null pointer / non-positive size */
  RRT_E_UNSUPPORTED = -2,   /* configuration outside the HIP path (see rrt_strerror) */
  RRT_E_WORKSPACE = -3,     /* workspace too small */
  RRT_E_HANDOVER = -4       /* an earlier merged R-MSA launch gave up its in-launch hand-over wait (rrt_device_error) */
};

/* Arithmetic of the nn.Linear layers (qkv / proj of R-MSA and CR-MSA, MLP phi).  F32 is exact
 * fp32 on the fp32 matrix cores (the default; what the <=1e-3 fp32 parity claim is made on).
 * BF16 / F16 round the two MFMA operands to bf16 / fp16 and accumulate in fp32 -- the
 * autocast-class numerics of the reference's --amp path (main.py:101-102,439); LayerNorm,
 * softmax statistics, residuals and the residual stream in HBM stay fp32 in every mode. */
enum { RRT_COMPUTE_F32 = 0, RRT_COMPUTE_BF16 = 1, RRT_COMPUTE_F16 = 2, RRT_COMPUTE_F32X3 = 3 };
/* F32X3 (inference): the qkv and proj GEMMs of the R-MSA layers -- 84 % of the FLOPs -- EMULATED in fp32 on the bf16
 * matrix cores: each fp32 operand is carried as a (hi, lo) pair of bf16 values (16 significant bits) and a product is
 * three bf16 MFMAs with fp32 accumulation, hi.hi + hi.lo + lo.hi.  Attention, LayerNorm, CR-MSA and every other GEMM
 * are the F32 path's.  Measured distance to the F32 path on the encoder output: ~1e-6; regions of 49..144
 * tokens with head dim 64, anything else silently takes the exact F32 kernels. */
/* In BF16 / F16 on regions of 17..256 tokens with head dim 64 the R-MSA layers run on 16-bit data end to end
 * (rrt_ln_partition16 -> rrt_rmsa_fused16 -> rrt_linear16_f32 below): the LayerNorm output, the weights and the
 * attention output live in HBM in 16 bits, and Q~, K, V and the softmax probabilities go to the matrix cores in 16
 * bits too (fp32 accumulation, fp32 softmax statistics) -- what autocast does to nn.Linear, q k^T and attn v.
 * The residual stream x / x1 / y, LayerNorm, CR-MSA's logits / combine / dispatch stay fp32. */
enum { RRT_POS_NONE = 0, RRT_POS_PEG = 1, RRT_POS_PPEG = 2 };
enum { RRT_EPEG_ATTN = 0, RRT_EPEG_VALUE_BF = 1, RRT_EPEG_VALUE_AF = 2 };

/* Elementwise activations of the caller-side layers (patch_to_emb, DAttention). */
enum { RRT_ACT_NONE = 0, RRT_ACT_RELU = 1, RRT_ACT_GELU = 2, RRT_ACT_TANH = 3, RRT_ACT_SIGMOID = 4 };

/* Region-grid geometry: RegionAttntion.padding, modules/rmsa.py:175-202 (same body
 * CrossRegionAttntion.padding :261-288).  H = padded grid side, s = region side,
 * add = zero rows appended (H*H - L). */
typedef struct rrt_grid {
  int64_t L;
  int32_t H;
  int32_t s;
  int32_t regions_side;
  int64_t add;
} rrt_grid;

/* Constructor surface that changes the arithmetic: RRTEncoder.__init__,
 * modules/rrt.py:134-163 (kwargs that reach TransLayer/InnerAttention). */
typedef struct rrt_encoder_desc {
  int32_t dim;             /* mlp_dim */
  int32_t n_heads;         /* n_heads (R-MSA), head_dim = dim / n_heads */
  int32_t n_rmsa_layers;   /* n_layers - 1 */
  int32_t region_num;      /* R-MSA regions per side */
  int32_t region_size;     /* >0 overrides region_num */
  int32_t min_region_num;
  float   min_region_ratio;
  int32_t epeg;            /* 1: 1-D 'attn' EPEG in the R-MSA layers */
  int32_t epeg_k;
  int32_t cr_msa;          /* 1: CR-MSA layer present */
  int32_t crmsa_k;
  int32_t crmsa_heads;
  int32_t crmsa_mlp;       /* 1: phi is Linear(dim, dim/4) -> Tanh -> Linear(dim/4, k), rmsa.py:248-252 */
  int32_t all_shortcut;
  int32_t compute;         /* RRT_COMPUTE_*: operand precision of the nn.Linear layers */
  int32_t ffn;             /* 1: every TransLayer (CR-MSA's too) ends with x + Mlp(LN2(x)), rrt.py:105-106,127-129 */
  int32_t ffn_act;         /* RRT_ACT_GELU (ffn_act='gelu') or RRT_ACT_RELU (anything else), rrt.py:105 */
  int32_t ffn_hidden;      /* int(dim * mlp_ratio), a multiple of 32 */
  int32_t pos;             /* RRT_POS_NONE / RRT_POS_PEG / RRT_POS_PPEG (pos=, modules/emb_position.py:24-82) */
  int32_t pos_pos;         /* -1: before the first layer; 0: before layer index 1 (needs n_layers >= 3), rrt.py:181-187 */
  int32_t peg_k;           /* odd, <= 11 */
  int32_t peg_1d;          /* 1: (k, 1) kernels (peg_1d / conv_1d) */
  /* EPEG ablations (rmsa.py:76-85,106-129; unfused path, forward and backward): */
  int32_t epeg_2d;         /* 1: k x k kernel -- over the score map ('attn') or over v's sqrt(P) x sqrt(P) image ('value_*') */
  int32_t epeg_type;       /* RRT_EPEG_ATTN (default) / RRT_EPEG_VALUE_BF / RRT_EPEG_VALUE_AF */
  /* Reduced-precision modes (BF16 / F16 / F32X3) keep 16-bit images of the R-MSA weights at the START of the workspace
   * (4 dim^2 floats per layer, whatever n_tokens is).  With 0 EVERY call in such a mode writes them (one launch,
   * ~5 us), whether or not this bag's region size takes the 16-bit kernels -- so "an earlier successful call on this
   * workspace with the same weights, dim, n_rmsa_layers and compute" is all that 1 has to promise; the bag sizes of
   * the two calls need not match.  The library keeps no state: 0 is always right, 1 is the caller's promise
   * (rrt_mil_amd tracks parameter versions). */
  int32_t weights16_valid;
  /* Scheduling hint.  Results are deterministic for a given setting and equal between the two settings up to fp32 summation
   * order: with 1 the representatives' two small GEMMs sum K in four interleaved groups (linear_splitk), so low-order
   * bits of the output may differ from a solo = 0 forward of the same bag (both within ~1e-6 of the float64 oracle); with 1 the
   * last R-MSA layer's merged launch also leaves CR-MSA's LayerNorm statistics / logit products (RRT_PLAN_CRMSA_PARTS), which
   * are then merged slab-wise instead of summed row-wise (same distance);
   * callers that compare bits across entry points use one setting (RRTEncoder.solo; the executor uses 0 unless it has
   * exactly one stream).  0 (default): other work may share the GPU with this forward (more bags in
   * flight on other streams): every kernel of the latency-bound CR-MSA tail keeps a footprint that fits NEXT TO a block
   * of the other bag's fused R-MSA kernel (<= 4 waves, <= 40 KiB LDS).  1: the forward has the GPU to itself (one bag in
   * flight): the representatives' small GEMMs may take whole CUs (16-wave blocks, K split inside the block: 10 -> 6-7 us
   * each).  The executor sets it to (n_streams == 1) itself. */
  int32_t solo;
} rrt_encoder_desc;

/* One TransLayer's parameters: InnerAttention, modules/rmsa.py:57-89 (+ the optional FFN).  Row-major, fp32.
 * qkv_w [3*dim, dim], qkv_b [3*dim] or NULL, proj_w [dim, dim], proj_b [dim],
 * pe_w [heads, epeg_k] or NULL, pe_b [heads] or NULL (epeg_2d: pe_w [heads, k, k]; epeg_type value_*:
 * pe_w [dim, k] or [dim, k, k], pe_b [dim] -- the value variants READ the bias, it is added to v / x). */
typedef struct rrt_attn_weights {
  const float *norm_w, *norm_b;   /* the owning TransLayer's LayerNorm, modules/rrt.py:47 */
  const float *qkv_w, *qkv_b;
  const float *proj_w, *proj_b;
  const float *pe_w, *pe_b;
  /* ffn = 1 only (Mlp, modules/rrt.py:25-41): norm2 [dim]; fc1 [ffn_hidden, dim] + [ffn_hidden];
   * fc2 [dim, ffn_hidden] + [dim] */
  const float *norm2_w, *norm2_b;
  const float *fc1_w, *fc1_b;
  const float *fc2_w, *fc2_b;
} rrt_attn_weights;

typedef struct rrt_encoder_weights {
  rrt_attn_weights rmsa[RRT_MAX_RMSA_LAYERS];   /* layers.{i}.* */
  rrt_attn_weights crmsa;                         /* cr_msa.norm.*, cr_msa.attn.attn.* */
  const float *phi;                               /* cr_msa.attn.phi [dim, crmsa_k]          (crmsa_mlp = 0) */
  const float *phi0_w, *phi2_w;                   /* cr_msa.attn.phi.0.weight [dim/4, dim],
                                                     cr_msa.attn.phi.2.weight [crmsa_k, dim/4] (crmsa_mlp = 1) */
  const float *norm_w, *norm_b;                   /* final norm.* (modules/rrt.py:139,195) */
  /* pos_embedding.proj / proj1 / proj2 (depth-wise [dim, 1, k, k] or [dim, 1, k, 1]; PEG: only [0]); biases may be
   * NULL (peg_bias = False) */
  const float *pos_w[3], *pos_b[3];
  /* 0 = unknown.  Otherwise a number the caller changes whenever any weight VALUE changes (the pointers alone do not
   * tell): the executor, which owns its workspaces, skips the 16-bit weight conversion of the reduced-precision modes
   * while it stays the same.  Stateless entry points ignore it (see rrt_encoder_desc.weights16_valid). */
  uint64_t version;
} rrt_encoder_weights;

int         rrt_abi_version(void);
const char *rrt_strerror(int code);          /* static string; also explains the last RRT_E_UNSUPPORTED of this thread */

/* host-only: modules/rmsa.py:175-202 */
int rrt_region_grid(int64_t L, int32_t region_num, int32_t region_size,
                    int32_t min_region_num, float min_region_ratio, rrt_grid *out);

/* host-only: bytes of workspace rrt_encoder_forward_f32 needs for a bag of n_tokens */
int rrt_encoder_workspace_size(const rrt_encoder_desc *desc, int64_t n_tokens, size_t *bytes);

/* host-only: which kernels rrt_encoder_forward_f32 takes for the R-MSA layers of a bag of n_tokens (for measurement:
 * bench.py attributes FLOPs to launches with it).  *flags = RRT_PLAN_* bits. */
#define RRT_PLAN_FUSED      1   /* qkv projection + EPEG + attention in one kernel per (region, head) (fp32 data) */
#define RRT_PLAN_FUSED_PROJ 2   /* ... with the out-projection + un-partition + residual as a later phase of the same launch */
#define RRT_PLAN_FUSED16    4   /* the 16-bit fused kernels (bf16 / fp16 modes) */
#define RRT_PLAN_FUSED_X3   8   /* the split-bf16 fused kernel (RRT_COMPUTE_F32X3) */
#define RRT_PLAN_CRMSA_PARTS 16 /* the last layer's merged launch also leaves CR-MSA's row records (LayerNorm 2 statistics +
                                   logit dot products); CR-MSA's first pass is rrt_crmsa_combine_parts_f32 */
#define RRT_PLAN_ATTN_HD    32  /* qkv linear + the MFMA attention forward at a head dim other than 64 (set alone; see
                                   rrt_region_attention_hd_supported) */
int rrt_encoder_plan(const rrt_encoder_desc *desc, int64_t n_tokens, int32_t *flags);
/* host-only: the form of the two streaming stages around the R-MSA layers (LayerNorm + partition; dispatch + final LayerNorm)
 * in the same forward.  *w = 0: one wave per token row; 1 .. 3: the row-looping kernels on a fixed grid of w waves per SIMD
 * (rrt_ln_partition_rows_f32, rrt_crmsa_dispatch_ln_rows_f32).  Same output bits either way. */
int rrt_encoder_plan_rows(const rrt_encoder_desc *desc, int64_t n_tokens, int32_t *w);

/* Whole path: RRTEncoder.forward, modules/rrt.py:165-202 (eval mode, one bag).
 * x [n_tokens, dim] -> y [n_tokens, dim]; x is not modified; y may not alias x. */
int rrt_encoder_forward_f32(const rrt_encoder_desc *desc, const rrt_encoder_weights *w,
                            const float *x, float *y, int64_t n_tokens,
                            void *workspace, size_t workspace_bytes, void *stream);

/* Test hook (tests/test_rows_kernels_gpu.py): the same forward with the form of its two streaming stages chosen by the caller
 * instead of the plan -- rows_w = 0: one wave per token row, 1 .. 3: the row-looping kernels at that width (see
 * rrt_encoder_plan_rows).  Every choice gives the same output bits. */
int rrt_debug_encoder_forward_rows_f32(const rrt_encoder_desc *desc, const rrt_encoder_weights *w,
                                       const float *x, float *y, int64_t n_tokens,
                                       void *workspace, size_t workspace_bytes, void *stream, int32_t rows_w);

/* Same call, recording caller-owned hipEvent_t's at stage boundaries on `stream` (for
 * measurement: bench.py times the dominant kernel with these).  events[RRT_EV_COUNT], any
 * entry may be NULL.  Only the first R-MSA layer is marked. */
enum {
  RRT_EV_START = 0,        /* before the first kernel */
  RRT_EV_LN_PARTITION,     /* after LayerNorm+partition */
  RRT_EV_QKV,              /* after the R-MSA qkv linear  (the dominant kernel) */
  RRT_EV_ATTN,             /* after the region attention core */
  RRT_EV_PROJ,             /* after proj + un-partition + residual */
  RRT_EV_CR_COMBINE,       /* after CR-MSA logits + combine */
  RRT_EV_CR_INNER,         /* after the inner MSA over the representatives */
  RRT_EV_END,              /* after dispatch + final LayerNorm */
  RRT_EV_COUNT
};
int rrt_encoder_forward_events_f32(const rrt_encoder_desc *desc, const rrt_encoder_weights *w,
                                   const float *x, float *y, int64_t n_tokens,
                                   void *workspace, size_t workspace_bytes, void *stream,
                                   void **events);

/* Concurrent forwards on several streams (one bag each): a phase gate shared by those calls keeps their
 * MFMA-bound R-MSA cores from co-running (they take turns instead of time-slicing the matrix pipes).  Optional:
 * pass gate = NULL for free-running streams, which measure faster with the current kernels (the executor below
 * gates only under RRT_GATE=1).  Host-side object, one host thread.  events may be NULL (else as in
 * rrt_encoder_forward_events_f32). */
typedef struct rrt_phase_gate rrt_phase_gate;
int rrt_phase_gate_create(rrt_phase_gate **out);
int rrt_phase_gate_destroy(rrt_phase_gate *gate);
int rrt_encoder_forward_gated_f32(const rrt_encoder_desc *desc, const rrt_encoder_weights *w,
                                  const float *x, float *y, int64_t n_tokens,
                                  void *workspace, size_t workspace_bytes, void *stream,
                                  rrt_phase_gate *gate, void **events);

/* Batch > 1: RRTEncoder.forward on (B, N, D) input (modules/rrt.py:165-202), inference.  x, y: [batch, n_tokens, dim]
 * contiguous.  At B > 1 the reference's region_partition puts the regions of all bags on one axis (rmsa.py:28-39): the R-MSA
 * layers still treat the bags independently, but CR-MSA's inner attention runs over the 64 * B representatives of ALL bags
 * (rmsa.py:316-322) -- the outputs of a batch differ from the outputs of its bags taken one at a time, and this entry point
 * reproduces exactly that.  (Independent bags -- what every reference trainer feeds, batch_size = 1 -- go through
 * rrt_encoder_forward_f32 / rrt_executor_forward.)  Correctness path: the R-MSA layers bag by bag, one inner MSA for the
 * batch; workspace from rrt_encoder_batch_workspace_size. */
int rrt_encoder_batch_workspace_size(const rrt_encoder_desc *desc, int32_t batch, int64_t n_tokens, size_t *bytes);
int rrt_encoder_forward_batch_f32(const rrt_encoder_desc *desc, const rrt_encoder_weights *w,
                                  const float *x, float *y, int32_t batch, int64_t n_tokens,
                                  void *workspace, size_t workspace_bytes, void *stream);

/* ---- stage entry points (what the fused path is built from; used by the parity tests) ---- */

/* LayerNorm (modules/rrt.py:121-123) + zero-pad (rmsa.py:199-200) + region_partition
 * (rmsa.py:28-39): x [L, dim] -> u [H*H, dim] in region-major order, pad rows = 0. */
int rrt_ln_partition_f32(const float *x, const float *gamma, const float *beta, float *u,
                         int64_t L, int32_t dim, const rrt_grid *g, void *stream);

/* The same stage in its row-looping form: a fixed grid of (device CUs x w) four-wave blocks, w = 1 .. 3 waves per SIMD, each
 * wave looping over token rows; u is bit-identical to rrt_ln_partition_f32's.  w = 0 runs the one-wave-per-row kernel.
 * zero / n_zero (may be NULL / 0): n_zero ints set to 0 as a side job, as the encoder uses it for arrival counters. */
int rrt_ln_partition_rows_f32(const float *x, const float *gamma, const float *beta, float *u,
                              int64_t L, int32_t dim, const rrt_grid *g, int32_t w,
                              int32_t *zero, int32_t n_zero, void *stream);

/* nn.Linear (rmsa.py:100, :131): C[M,N] = A[M,K] . B[N,K]^T + bias[N] (bias may be NULL).
 * q_cols>0: columns [0,q_cols) are multiplied by q_scale after the bias (rmsa.py:103). */
int rrt_linear_f32(const float *A, const float *B, const float *bias, float *C,
                   int64_t M, int32_t N, int32_t K, int32_t q_cols, float q_scale,
                   int32_t compute /* RRT_COMPUTE_* */, void *stream);

/* nn.Linear + region_reverse + un-pad + residual (rmsa.py:131, :41-54, :227-228; rrt.py:125):
 * out[t] = resid[t] + (A . B^T + bias)[slot(t)] for the L real tokens. */
int rrt_linear_unpartition_residual_f32(const float *A, const float *B, const float *bias,
                                        const float *resid, float *out, int32_t N, int32_t K,
                                        const rrt_grid *g, int32_t compute, void *stream);

/* The kernel form one GEMM of this library takes (exports added under ABI 29, no existing struct or signature touched).
 * Host only, nothing is launched; the answer comes from the function the launchers of csrc/linear_f32.hip dispatch from
 * (plan_linear), so it cannot drift from what runs.  tests/test_linear_form_matrix.py asserts the form of every case with it
 * and tests/test_linear_form_grid_cpu.py sweeps it against the instantiations that file compiles.
 *   operands  RRT_LINEAR_OPS_F32   fp32 operands in memory (compute = RRT_COMPUTE_F32 / BF16 / F16 rounds them after LDS)
 *             RRT_LINEAR_OPS_16    16-bit images (rrt_cast16; compute = RRT_COMPUTE_BF16 / F16), K % 64 == 0
 *             RRT_LINEAR_OPS_SPLIT split images (rrt_cast_split; compute = RRT_COMPUTE_F32X3)
 *   epilogue  RRT_LINEAR_EPI_*: plain (bias, q-scale), activation, un-partition + residual, dropout (fp32 training), both
 *   solo      the scheduling hint of rrt_encoder_desc.solo;  zero64: the 64-counter side job is set
 * plan[RRT_LINEAR_PLAN_INTS]: [0] kernel RRT_LINEAR_KERNEL_*, [1] MT, [2] NT (block tile = 16 MT x 64 NT), [3] cap of the
 * persistent grid (0 for split-K), [4] tiles, [5] grid, [6] 1 = the warp-specialised kernel's deferred-epilogue instantiation,
 * [7] split-K: K groups per block (else 0), [8] split-K: 1 = the dropout instantiation, [9] epilogue of the instantiation
 * (RRT_LINEAR_EPI_*), [10] MFMA operand precision of the instantiation (RRT_COMPUTE_*), [11] 0.
 * What the kernel itself decides from its arguments (the straight-line un-partition store: N % (64 NT) == 0 and q_cols == 0;
 * the 32-bit byte-offset limit of the buffer stores) is not reported.  RRT_E_UNSUPPORTED for what the launchers refuse. */
enum { RRT_LINEAR_OPS_F32 = 0, RRT_LINEAR_OPS_16 = 1, RRT_LINEAR_OPS_SPLIT = 2 };
enum { RRT_LINEAR_EPI_PLAIN = 0, RRT_LINEAR_EPI_UNPART = 1, RRT_LINEAR_EPI_ACT = 2, RRT_LINEAR_EPI_UNPART_DROP = 3,
       RRT_LINEAR_EPI_DROP = 4 };
enum { RRT_LINEAR_KERNEL_PLAIN = 0, RRT_LINEAR_KERNEL_WS = 1, RRT_LINEAR_KERNEL_SPLITK = 2 };
#define RRT_LINEAR_PLAN_INTS 12
int rrt_linear_plan(int64_t M, int32_t N, int32_t K, int32_t compute, int32_t operands, int32_t epilogue,
                    int32_t solo, int32_t zero64, int32_t *plan);

/* Stage entry for tests: one GEMM with the WHOLE epilogue the forwards can ask for, so that every kernel form plan_linear can
 * pick is reachable at a small shape (the rrt_linear*_f32 entries above and below never set solo, dropout or zero64).
 * A, B: fp32 [M, K] / [N, K], or 16-bit / split images of them, per `operands`; bias [N] or NULL; columns [0, q_cols) times
 * q_scale after the bias; act = RRT_ACT_*; resid (may be NULL) [g->L, N] with g: C row = token, A row = slot, M == g->H^2;
 * drop_p > 0: the training forward's dropout epilogue, threshold, scale and seed derived from (drop_p, drop_seed, drop_layer)
 * exactly as rrt_encoder_forward_train_f32 derives them for R-MSA layer drop_layer (100: CR-MSA); zero64 (may be NULL): 64
 * ints that block 0 sets to 0.  Launches what the launchers launch and nothing else; RRT_E_INVALID on NULL / non-positive /
 * inconsistent arguments, RRT_E_UNSUPPORTED where the launchers refuse (dropout outside exact fp32 or with an activation, an
 * activation together with resid or on split images, K not a multiple of 32 / 64). */
int rrt_debug_linear_f32(const void *A, const void *B, const float *bias, const float *resid, float *C,
                         int64_t M, int32_t N, int32_t K, const rrt_grid *g, int32_t operands, int32_t compute,
                         int32_t q_cols, float q_scale, int32_t act, int32_t solo,
                         float drop_p, uint64_t drop_seed, int32_t drop_layer, int32_t *zero64, void *stream);

/* Region attention core (rmsa.py:103-122): qkv [n_regions*P, 3*dim] (q already scaled),
 * EPEG taps pe_w [heads, epeg_k] (NULL/0 = none; pe bias is softmax-invariant and not needed)
 * -> o [n_regions*P, dim] (heads merged).
 * Which kernel runs, by head dim = dim / heads: 64 -> the head-dim-64 MFMA kernels; every other multiple of 16 in
 * [16, 256] with epeg_k <= 63 -> the MFMA kernel of rrt_region_attention_hd_f32; anything else (above 256, not a
 * multiple of 16) -> a VALU kernel, one wave per query. */
int rrt_region_attention_f32(const float *qkv, const float *pe_w, float *o,
                             int32_t n_regions, int32_t P, int32_t dim, int32_t heads,
                             int32_t epeg_k, void *stream);

/* host-only: 1 when rrt_region_attention_f32 takes the MFMA kernel for head dims other than 64, else 0:
 * heads divides dim, dim / heads is a multiple of 16 in [16, 256] and not 64, epeg_k <= 63, any P >= 1. */
int rrt_region_attention_hd_supported(int32_t P, int32_t dim, int32_t heads, int32_t epeg_k);
/* That kernel alone (same arguments and result as rrt_region_attention_f32): RRT_E_UNSUPPORTED outside the predicate
 * above -- checked before the pointers, which are not touched then -- and RRT_E_INVALID on NULL qkv / o. */
int rrt_region_attention_hd_f32(const float *qkv, const float *pe_w, float *o,
                                int32_t n_regions, int32_t P, int32_t dim, int32_t heads,
                                int32_t epeg_k, void *stream);

/* Fused R-MSA core (rmsa.py:100-122 in one kernel per (region, head)): u [n_regions*P, dim]
 * region-major LayerNorm-ed tokens -> o [n_regions*P, dim]; qkv_w [3*dim, dim], qkv_b [3*dim] or NULL,
 * pe_w [heads, epeg_k] or NULL.  The qkv tensor never exists in HBM.  Supported when head dim is 64
 * and 48 < P <= 208 (one region's Q, K, V tiles fit a CU's LDS); otherwise RRT_E_UNSUPPORTED and the caller uses
 * rrt_linear_f32 + rrt_region_attention_f32 (rrt_encoder_forward_f32 chooses by itself). */
int rrt_rmsa_fused_f32(const float *u, const float *qkv_w, const float *qkv_b, const float *pe_w,
                       float *o, int32_t n_regions, int32_t P, int32_t dim, int32_t heads,
                       int32_t epeg_k, int32_t compute, void *stream);

/* The same kernel with the out-projection as a later phase of the SAME launch (fp32 exact): rrt_rmsa_fused_f32 followed by
 * rrt_linear_unpartition_residual_f32 in one launch, bit-identical to that pair --
 * out[t] = resid[t] + (o . proj_w^T + proj_b)[slot(t)] (rmsa.py:100-131, :41-54, :227-228; rrt.py:125).
 * u [H*H, dim] region-major (rrt_ln_partition_f32 on g); o_scratch: H*H*dim floats (the attention output, device scratch);
 * counters: regions_side^2 int32 of device scratch (zeroed by the call).  Needs regions of > 64 tokens and heads * regions >= 2 x the CU count
 * (block b of the launch runs (region, head) item b and then the 64-column projection slab b - CUs of a region whose
 * items finished a whole item earlier), otherwise RRT_E_UNSUPPORTED; rrt_encoder_forward_f32 chooses by itself. */
int rrt_rmsa_fused_proj_f32(const float *u, const float *qkv_w, const float *qkv_b, const float *pe_w,
                            const float *proj_w, const float *proj_b, const float *resid, float *out,
                            float *o_scratch, int32_t *counters, int32_t dim, int32_t heads, int32_t epeg_k,
                            const rrt_grid *g, void *stream);
/* ... and CR-MSA's first pass as a by-product (what rrt_encoder_forward_f32 does for the LAST R-MSA layer when a plain-phi
 * CR-MSA with k <= 4 follows it directly and desc.solo != 0 -- it trades ~3 us of the merged launch's matrix-pipe time for
 * ~6 us of latency-bound CR-MSA front: a gain with one bag in flight, none with four): out = x1 is CR-MSA's input, and the slabs hold its tiles in registers -- per (token t,
 * 64-column slab c) they also store the record  part[(t * dim / 64 + c) * S ..] = (mean, M2, d_0 .. d_k-1), S = 2 + k rounded
 * up to a multiple of 4:  mean and
 * centred sum of squares of x1[t, 64 c .. 64 c + 63], d_n = sum_j x1[t, j] ln2_gamma[j] phi[j, n] over those columns
 * (LayerNorm 2 = cr_msa.norm, phi [dim, k] = cr_msa.attn.phi; modules/rmsa.py:303-307, rrt.py:121).  part: n_tokens * dim / 64 *
 * S floats of device scratch (dim <= 512).  rrt_crmsa_combine_parts_f32 turns them and ONE pass over x1 into CR-MSA's combine:
 * logits / region softmax / min-max / dispatch weights wdisp [H8*H8, k] (region-major) and the representatives
 * rep [k, 64, dim] (rmsa.py:307-316) -- the job of rrt_crmsa_logits_f32 + rrt_crmsa_combine_f32, without re-reading x1 for
 * LayerNorm and without any hand-over between blocks.  g8 = rrt_region_grid(n_tokens, 8, ...). */
int rrt_rmsa_fused_proj_stats_f32(const float *u, const float *qkv_w, const float *qkv_b, const float *pe_w,
                                  const float *proj_w, const float *proj_b, const float *resid, float *out,
                                  float *o_scratch, int32_t *counters, const float *ln2_gamma, const float *phi,
                                  int32_t crmsa_k, float *part, int32_t dim, int32_t heads, int32_t epeg_k,
                                  const rrt_grid *g, void *stream);
int rrt_crmsa_combine_parts_f32(const float *x1, const float *part, const float *gamma, const float *beta,
                                const float *phi, float *wdisp, float *rep, int64_t n_tokens, int32_t dim, int32_t k,
                                const rrt_grid *g8, void *stream);
/* The in-launch hand-over of that kernel and what it assumes.  A projection slab (block b >= lag) spins on its region's
 * arrival counter until the region's `heads` items -- blocks with LOWER indices -- have stored their O rows.  Forward
 * progress rests on the GPU dispatching the workgroups of one launch in index order (so an awaited item is running or
 * done when its slab starts): observed on every gfx9 part, relied on here, but NOT an architectural guarantee.  The wait
 * is therefore bounded (2^22 sleeps of ~0.2 us, about a second): a slab that gives up writes nothing and raises the
 * process's hand-over error word (pinned host memory, no device sync needed to read it).  From then on
 * rrt_encoder_forward_* / rrt_mil_forward_f32 / rrt_executor_forward / rrt_rmsa_fused_proj_f32 return RRT_E_HANDOVER
 * without launching anything, until the caller has looked at it:
 *   rrt_device_error(clear): 0, or 1 + the region whose slab gave up; clear != 0 resets the word (after the caller has
 *   synchronised the device and discarded the outputs of the forwards in flight).  This word is the library's only state. */
int rrt_device_error(int32_t clear);
/* Test hook for that path (tests/test_hip_parity.py): rrt_rmsa_fused_proj_f32 with a caller-chosen lag (0: the rule;
 * otherwise 8 * heads <= lag <= heads * regions; a lag that is not a multiple of 8 puts every slab on ANOTHER XCD than
 * the items it reads -- the hand-over must not depend on the placement heuristic), spin limit (0: 2^22) and
 * `wait_extra` arrivals more than a region ever gets (> 0: every slab times out -- exercises the error path). */
int rrt_debug_rmsa_fused_proj_f32(const float *u, const float *qkv_w, const float *qkv_b, const float *pe_w,
                                  const float *proj_w, const float *proj_b, const float *resid, float *out,
                                  float *o_scratch, int32_t *counters, int32_t dim, int32_t heads, int32_t epeg_k,
                                  const rrt_grid *g, int32_t lag, int32_t spin_limit, int32_t wait_extra, void *stream);

/* 16-bit operand stages of the reduced-precision modes (compute = RRT_COMPUTE_BF16 / F16 selects the element type;
 * uint16_t* = raw bf16 / fp16 bits, round-to-nearest-even):
 *  cast16        : dst[i] = (16-bit) src[i], n % 4 == 0 (the nn.Linear weights, once per forward);
 *  ln_partition16: rrt_ln_partition_f32 with the normalised rows rounded to 16 bits (what autocast feeds nn.Linear);
 *  linear16      : C fp32 [M, N] = A16 [M, K] . B16 [N, K]^T + bias; with resid != NULL the un-partition + residual
 *                  epilogue of rrt_linear_unpartition_residual_f32 (M = H*H of g); K % 64 == 0 (any M: ragged
 *                  row tiles are masked);
 *  rmsa_fused16  : rrt_rmsa_fused_f32 on 16-bit u / qkv_w, attention operands in 16 bits, o in 16 bits
 *                  (rmsa.py:100-122 under autocast); head dim 64, 16 < P <= 256. */
int rrt_cast16(const float *src, uint16_t *dst, int64_t n, int32_t compute, void *stream);
int rrt_ln_partition16(const float *x, const float *gamma, const float *beta, uint16_t *u, int64_t L,
                       int32_t dim, const rrt_grid *g, int32_t compute, void *stream);
int rrt_linear16_f32(const uint16_t *A, const uint16_t *B, const float *bias, const float *resid, float *C,
                     int64_t M, int32_t N, int32_t K, const rrt_grid *g, int32_t compute, void *stream);
int rrt_rmsa_fused16(const uint16_t *u, const uint16_t *qkv_w, const float *qkv_b, const float *pe_w,
                     uint16_t *o, int32_t n_regions, int32_t P, int32_t dim, int32_t heads, int32_t epeg_k,
                     int32_t compute, void *stream);
/* Round 6: rrt_rmsa_fused16 + rrt_linear16_f32(resid) of one R-MSA layer in ONE launch (modules/rmsa.py:100-132, :41-54,
 * :227-228; rrt.py:125 under autocast), what rrt_encoder_forward_f32 uses in BF16 / F16 for bags of at least two rounds of
 * (region pair, head) items -- regions of 65..96 or 113..128 tokens, a multiple of 16 regions, e.g. N = 30000 at
 * region_num = 16: block b runs item b and then the 64-column projection slab b - 256 of a pair whose items finished a
 * round earlier; out [L, dim] = resid + unpartition(o proj_w^T + proj_b), bit-identical to the two calls; o [Np, dim] is
 * scratch (the 16-bit attention output); cnt: Np / (2 P) ints of scratch (zeroed by the call).  The in-launch hand-over is
 * bounded like rrt_rmsa_fused_proj_f32's (RRT_E_HANDOVER, rrt_device_error). */
int rrt_rmsa_pair16_proj(const uint16_t *u, const uint16_t *qkv_w, const float *qkv_b, const float *pe_w,
                         const uint16_t *proj_w, const float *proj_b, const float *resid, float *out, uint16_t *o,
                         int32_t *cnt, int32_t dim, int32_t heads, int32_t epeg_k, const rrt_grid *g, int32_t compute,
                         void *stream);

/* RRT_COMPUTE_F32X3 stages.  A "split image" of a row-major fp32 array holds, per 32 consecutive elements, 32 bf16 hi
 * values then 32 bf16 lo values (128 bytes; hi = bf16(x), lo = bf16(x - hi)) -- 4 bytes per element like the original.
 *  cast_split        : dst = split image of src, n % 32 == 0 (the weights, once per forward);
 *  ln_partition_split: rrt_ln_partition_f32 with the rows written as a split image;
 *  linear_split      : C fp32 [M, N] = A . B^T + bias from split images of A [M, K] and B [N, K]; with resid != NULL
 *                      the un-partition + residual epilogue (M = H*H of g); K % 32 == 0;
 *  rmsa_fused_x3     : rrt_rmsa_fused_f32 on split images of u / qkv_w, o written as a split image; 48 < P <= 144. */
int rrt_cast_split(const float *src, void *dst, int64_t n, void *stream);
int rrt_ln_partition_split(const float *x, const float *gamma, const float *beta, void *u, int64_t L,
                           int32_t dim, const rrt_grid *g, void *stream);
int rrt_linear_split_f32(const void *A, const void *B, const float *bias, const float *resid, float *C,
                         int64_t M, int32_t N, int32_t K, const rrt_grid *g, void *stream);
int rrt_rmsa_fused_x3(const void *u, const void *qkv_w, const float *qkv_b, const float *pe_w, void *o,
                      int32_t n_regions, int32_t P, int32_t dim, int32_t heads, int32_t epeg_k, void *stream);

/* CR-MSA (rmsa.py:303-335), three kernels around the inner MSA (g8 = the 8x8 grid):
 *  logits  : LayerNorm statistics mean_rstd [L,2] and logits [Np8, k] in region-major order
 *            (zero rows for pad tokens);
 *  combine : per region the combine softmax over its P tokens -> rep [k, R8, dim], and the
 *            per-token dispatch weights wdisp [Np8, k] = minmax_p(logit) * softmax_k(logit);
 *            with mean_rstd == NULL, x1 must already hold LN(x1) in region-major order
 *            [Np8, dim] (the crmsa_mlp path) and gamma/beta are ignored;
 *  dispatch: y = LN(x1 + sum_n wdisp[.,n] * rep2[n, region] (+ x0)), the final norm fused. */
int rrt_crmsa_logits_f32(const float *x1, const float *gamma, const float *beta, const float *phi,
                         float *mean_rstd, float *logits, int64_t L, int32_t dim, int32_t k,
                         const rrt_grid *g8, void *stream);
int rrt_crmsa_combine_f32(const float *x1, const float *gamma, const float *beta,
                          const float *mean_rstd, const float *logits, float *wdisp, float *rep,
                          int64_t L, int32_t dim, int32_t k, const rrt_grid *g8, void *stream);
/* logits + combine in one pass over x1 (dim = 512, k <= 3, CR-MSA regions of <= 144 tokens: one block per region, the rows
 * are read once and stay in registers; rrt_encoder_forward_f32 uses it under RRT_CRMSA_REGION=1 -- better with several
 * bags in flight, worse with one); same outputs as the two calls above
 * (mean_rstd and logits may be NULL); RRT_E_UNSUPPORTED outside that range. */
int rrt_crmsa_region_f32(const float *x1, const float *gamma, const float *beta, const float *phi,
                         float *mean_rstd, float *logits, float *wdisp, float *rep,
                         int64_t L, int32_t dim, int32_t k, const rrt_grid *g8, void *stream);
/* The same at full chip width, what rrt_encoder_forward_f32 uses (dim = 512, k <= 8, regions of 4..576 tokens -- bags up
 * to ~36 k patches --, at least one R-MSA layer): 4 / 8 / 16 blocks per region (regions of <= 144 / 288 / 576 tokens), each
 * with its share of the rows; the block that arrives last merges the partial records like an online softmax (nobody
 * waits for anybody).  scratch: 256 + 64 * nb * km * 520 * 4 bytes with nb = 16 for regions of more than 288 tokens, else
 * 8, and km = 3 for k <= 3, else 8; logits must be given (the merging block reads them); mean_rstd may be NULL. */
int rrt_crmsa_region4_f32(const float *x1, const float *gamma, const float *beta, const float *phi,
                          float *mean_rstd, float *logits, float *wdisp, float *rep,
                          int64_t L, int32_t dim, int32_t k, const rrt_grid *g8,
                          void *scratch, size_t scratch_bytes, void *stream);
/* Round 6: the one-pass form for LARGER regions (what rrt_encoder_forward_f32 uses above 144 tokens per CR-MSA region, i.e.
 * bags of more than ~9.2 k patches: replaces modules/rmsa.py:303-316 like the two calls at the top of this group, reading x1
 * once instead of twice): always 4 blocks per region, each STREAMING its quarter of the rows in trips with a per-wave online
 * softmax; records, merge, scratch layout and arguments exactly as rrt_crmsa_region4_f32 (dim = 512, k <= 8, regions of
 * 16..576 tokens). */
int rrt_crmsa_stream4_f32(const float *x1, const float *gamma, const float *beta, const float *phi,
                          float *mean_rstd, float *logits, float *wdisp, float *rep,
                          int64_t L, int32_t dim, int32_t k, const rrt_grid *g8,
                          void *scratch, size_t scratch_bytes, void *stream);
int rrt_crmsa_dispatch_ln_f32(const float *x1, const float *x0, const float *wdisp,
                              const float *rep2, const float *gamma,
                              const float *beta, float *y, int64_t L, int32_t dim, int32_t k,
                              const rrt_grid *g8, void *stream);
/* rrt_crmsa_dispatch_ln_f32 in its row-looping form (w = 1 .. 3 as rrt_ln_partition_rows_f32; w = 0: the one-wave-per-row
 * kernel): y is bit-identical.  y16 (may be NULL): the output rows once more as 16-bit values, prec16 = RRT_COMPUTE_BF16 /
 * RRT_COMPUTE_F16 (the slide classifier's side output).  k = 0 with wdisp = rep2 = y16 = NULL (g8 ignored): the plain
 * LayerNorm of x1 (+ x0) that rrt_layernorm_f32 runs, in the chosen form. */
int rrt_crmsa_dispatch_ln_rows_f32(const float *x1, const float *x0, const float *wdisp,
                                   const float *rep2, const float *gamma,
                                   const float *beta, float *y, int64_t L, int32_t dim, int32_t k,
                                   const rrt_grid *g8, int32_t w, uint16_t *y16, int32_t prec16, void *stream);
/* crmsa_mlp logits (rmsa.py:248-252, :305): logits[r, n] = sum_j tanh(hid[r, j]) * w2[n, j] */
int rrt_crmsa_mlp_logits_f32(const float *hid, const float *w2, float *logits, int64_t rows,
                             int32_t hdim, int32_t k, void *stream);
/* final LayerNorm only (cr_msa=False path): y = LN(x1 (+ x0)) */
int rrt_layernorm_f32(const float *x1, const float *x0, const float *gamma, const float *beta,
                      float *y, int64_t L, int32_t dim, void *stream);

/* ---- row f1: the RRTMIL slide classifier around the encoder (modules/rrt.py:204-246) ----
 * patch_to_emb Linear(input_dim, dim)+act (rrt.py:208-217; Dropout is identity in eval) ->
 * RRTEncoder -> DAttention pooling (modules/datten.py) -> predictor Linear(dim, n_classes). */
typedef struct rrt_mil_desc {
  rrt_encoder_desc enc;
  int32_t input_dim;       /* patch feature width (multiple of 32) */
  int32_t emb_act;         /* RRT_ACT_RELU / RRT_ACT_GELU / RRT_ACT_NONE (RRTMIL act=) */
  int32_t n_classes;
  int32_t pool_hidden;     /* DAttention D = 128 (multiple of 4) */
  int32_t pool_act;        /* RRT_ACT_RELU / GELU / TANH / NONE (da_act) */
  int32_t pool_gated;      /* 1: AttentionGated (datten.py:40-83) */
  int32_t input16;         /* (ABI 25) 0: x is fp32.  RRT_COMPUTE_BF16 / RRT_COMPUTE_F16: x points to 16-bit features of that
                            * type [n_tokens, input_dim] (half the PCIe / HBM bytes of the bag, rrt_mil_amd.BagFeeder(dtype=...));
                            * needs enc.compute == input16 and input_dim % 64 == 0, otherwise RRT_E_UNSUPPORTED.  Under autocast
                            * the reference's first op (patch_to_emb Linear, rrt.py:208-229) rounds the fp32 features to exactly
                            * these 16-bit values, so the logits are bit-identical to the fp32-fed call. */
} rrt_mil_desc;

/* Row-major fp32, state_dict layout.  Non-gated: pool_a = pool_fn.attention.attention.0,
 * pool_c = its last Linear; gated: pool_a/pool_b/pool_c = attention_a.0 / attention_b.0 / attention_c.
 * Biases may be NULL (da_bias=False). */
typedef struct rrt_mil_weights {
  rrt_encoder_weights enc;
  const float *emb_w, *emb_b;         /* patch_to_emb.0  [dim, input_dim], [dim] */
  const float *pool_a_w, *pool_a_b;   /* [pool_hidden, dim], [pool_hidden] */
  const float *pool_b_w, *pool_b_b;   /* gated only */
  const float *pool_c_w, *pool_c_b;   /* [1, pool_hidden], [1] */
  const float *pred_w, *pred_b;       /* predictor [n_classes, dim], [n_classes] */
} rrt_mil_weights;

/* The pooling alone (datten.py:28-38 / :69-83 AFTER the first Linear + activation; training keeps those as autograd-visible
 * layers): s_n = c_w . h_n + c_b with h = hid_a (or hid_a * hid_b, gated), attn = softmax_n(s), pooled = sum_n attn_n y_n.
 * Outputs pooled [dim], attn [N] (normalised), a_raw [N] (the scores).  ... and its adjoint: given d_pooled [dim] (and
 * optionally d_attn [N] with c_ext = sum_n attn_n d_attn_n as a device scalar, d_raw [N]) ->
 * dy [N, dim] = attn_n d_pooled, dhid_a / dhid_b [N, hidden], dwcb [hidden + 4] = d c_w | d c_b (at [hidden]).
 * workspace: rrt_attn_pool_workspace_size bytes (either call).
 * Limits (RRT_E_UNSUPPORTED from the size query and from both calls alike, before anything is launched): dim % 32, hidden % 4,
 * n_tokens <= 1e6; the merge block's LDS 4 * (n_tokens / 32 + dim) + 16 KB <= 150 KB; the backward block's LDS
 * 4 * (dim + 4 * (hidden + 4)) <= 64 KB. */
int rrt_attn_pool_workspace_size(int64_t n_tokens, int32_t dim, int32_t hidden, size_t *bytes);
int rrt_attn_pool_f32(const float *y, const float *hid_a, const float *hid_b, const float *c_w, const float *c_b,
                      float *pooled, float *attn, float *a_raw, int64_t n_tokens, int32_t dim, int32_t hidden,
                      void *workspace, size_t workspace_bytes, void *stream);
int rrt_attn_pool_backward_f32(const float *y, const float *hid_a, const float *hid_b, const float *c_w,
                               const float *attn, const float *pooled, const float *d_pooled,
                               const float *d_attn, const float *d_raw, const float *c_ext, float *dy,
                               float *dhid_a, float *dhid_b, float *dwcb, int64_t n_tokens, int32_t dim,
                               int32_t hidden, void *workspace, size_t workspace_bytes, void *stream);

int rrt_mil_workspace_size(const rrt_mil_desc *desc, int64_t n_tokens, size_t *bytes);

/* RRTMIL.forward (eval, one bag): x [n_tokens, input_dim] -> logits [n_classes].
 * attn (optional, [n_tokens]): the attention row the reference returns with return_attn=True
 * (softmax over the bag, or the raw scores when no_norm != 0).  feat (optional, [n_tokens, dim]):
 * the encoder output. */
int rrt_mil_forward_f32(const rrt_mil_desc *desc, const rrt_mil_weights *w, const float *x,
                        float *logits, float *attn, int32_t no_norm, float *feat, int64_t n_tokens,
                        void *workspace, size_t workspace_bytes, void *stream);

/* DAttention + predictor alone on encoder features y [n_tokens, dim] (datten.py:28-38,69-83; rrt.py:241).
 * pooled (optional, [dim]) receives the bag embedding.  workspace: rrt_pool_workspace_size bytes.
 * Limits as rrt_attn_pool_f32's forward (the merge block's LDS <= 150 KB); rrt_mil_* and rrt_bagmil_* with an attention pool
 * refuse the same shapes from their size queries and their forwards. */
int rrt_pool_workspace_size(int64_t n_tokens, int32_t dim, int32_t hidden, int32_t gated, size_t *bytes);
int rrt_pool_predict_f32(const float *y, const float *a_w, const float *a_b, const float *b_w,
                         const float *b_b, const float *c_w, const float *c_b, const float *pred_w,
                         const float *pred_b, float *pooled, float *logits, float *attn, int32_t no_norm,
                         int64_t n_tokens, int32_t dim, int32_t hidden, int32_t act, int32_t n_classes,
                         int32_t compute, void *workspace, size_t workspace_bytes, void *stream);

/* nn.Linear with an activation epilogue: C = act(A . B^T + bias)   (patch_to_emb, rrt.py:208-217) */
int rrt_linear_act_f32(const float *A, const float *B, const float *bias, float *C, int64_t M, int32_t N,
                       int32_t K, int32_t act, int32_t compute, void *stream);

/* ---- CLAM_SB / CLAM_MB heads (modules/clam.py; ABI 29): multi-branch gated attention pooling ----
 * The branch pool alone (clam.py:25-74 AFTER the first Linear + activation, :172-177, :203 / :293): K attention branches
 * from ONE pass over y --
 *     s[c, n] = c_w[c] . h_n + c_b[c]   (h = hid_a, or hid_a * hid_b when hid_b != NULL),
 *     attn[c, :] = softmax_n(s[c, :]),   pooled[c, :] = sum_n attn[c, n] y_n.
 * y [N, dim], hid_a / hid_b [N, hidden], c_w [K, hidden], c_b [K] or NULL.  Outputs: pooled [K, dim], a_raw [K, N] (the
 * scores), attn [K, N] (optional, may be NULL).  1 <= K <= 8, dim % 32 == 0, dim <= 2048, hidden % 4 == 0, N <= 1e6,
 * otherwise RRT_E_UNSUPPORTED (inside these limits the merge block's LDS, 4 * (N / 32 + dim) bytes + 16 KiB, always fits).
 * Every sum has a fixed order: the same inputs give the same bits.
 * ... and its adjoint: given d_pooled [K, dim] and optionally d_raw [K, N] -> dy [N, dim], dhid_a / dhid_b [N, hidden],
 * dwcb [K * hidden + 8] = d c_w [K, hidden] | d c_b [K] (at [K * hidden]).  The adjoint alone has one more limit: its block
 * keeps d_pooled and four d c_w partials in LDS, K * (dim + 4 * hidden) + 32 floats <= 150 KiB, otherwise
 * RRT_E_UNSUPPORTED (the forward and the workspace query do not have it; CLAM's K <= 8, dim 512, hidden <= 384 need 65 KiB).
 * workspace: rrt_branch_pool_workspace_size bytes (either call). */
int rrt_branch_pool_workspace_size(int64_t n_tokens, int32_t dim, int32_t hidden, int32_t n_branches, size_t *bytes);
int rrt_branch_pool_f32(const float *y, const float *hid_a, const float *hid_b, const float *c_w, const float *c_b,
                        float *pooled, float *attn, float *a_raw, int64_t n_tokens, int32_t dim, int32_t hidden,
                        int32_t n_branches, void *workspace, size_t workspace_bytes, void *stream);
int rrt_branch_pool_backward_f32(const float *y, const float *hid_a, const float *hid_b, const float *c_w,
                                 const float *attn, const float *pooled, const float *d_pooled, const float *d_raw,
                                 float *dy, float *dhid_a, float *dhid_b, float *dwcb, int64_t n_tokens, int32_t dim,
                                 int32_t hidden, int32_t n_branches, void *workspace, size_t workspace_bytes,
                                 void *stream);

/* Top-k instance selection (the torch.topk calls of clam.py:141-143, :161): for each of n_rows rows of n floats,
 * idx [n_rows, 2, k] (int64) = the indices of the k largest values in descending order ([r, 0, :]) and of the k smallest
 * in ascending order ([r, 1, :]).  TIES: among equal values the LOWER index comes first, at both ends (torch leaves the
 * order of ties unspecified).  NaN entries are never selected; a row with fewer than k non-NaN values has its unused slots
 * set to -1.  1 <= k <= 32 (else RRT_E_UNSUPPORTED), n < k is RRT_E_INVALID, n <= 2^31 - 2, n_rows <= 65535. */
int rrt_topk_rows_f32(const float *x, int64_t *idx, int32_t n_rows, int64_t n, int32_t k, void *stream);

/* CLAM_SB / CLAM_MB.forward (eval, one bag, one stream): x [n_tokens, input_dim] -> Linear(input_dim, dim) + act ->
 * RRTEncoder (has_rrt; the reference allows rrt=None) -> the two gate Linears tanh / sigmoid (enc.compute's arithmetic)
 * -> branch pool -> bag logits [n_classes]. */
typedef struct rrt_clam_desc {
  rrt_encoder_desc enc;    /* has_rrt = 0: only dim (= 512 in the reference) and compute are read */
  int32_t input_dim;       /* patch feature width (multiple of 32) */
  int32_t emb_act;         /* RRT_ACT_RELU / RRT_ACT_GELU */
  int32_t has_rrt;         /* 1: the encoder sits between the embedding and the attention net (clam.py:104-105) */
  int32_t n_classes;
  int32_t per_branch;      /* 0: CLAM_SB, one branch, logits = cls_w [n_classes, dim] . M[0] + cls_b;
                            * 1: CLAM_MB, n_classes branches, logits[c] = cls_w[c] . M[c] + cls_b[c] */
  int32_t gated;           /* 1: Attn_Net_Gated */
  int32_t hidden;          /* gate width: 256 ('small') / 384 ('big'); a multiple of 4 */
  int32_t k_sample;        /* width of topk_idx (1..32; read only when topk_idx != NULL) */
} rrt_clam_desc;

typedef struct rrt_clam_weights {
  rrt_encoder_weights enc;
  const float *emb_w, *emb_b;         /* attention_net.0        [dim, input_dim], [dim] */
  const float *a_w, *a_b;             /* attention_a.0 / module.0   [hidden, dim], [hidden] */
  const float *b_w, *b_b;             /* attention_b.0 (gated only) */
  const float *c_w, *c_b;             /* attention_c / module's last Linear  [K, hidden], [K]   (K = per_branch ? n_classes : 1) */
  const float *cls_w, *cls_b;         /* SB: classifiers [n_classes, dim], [n_classes]; MB: the n_classes Linear(dim, 1)
                                       * rows packed by the caller into [n_classes, dim], [n_classes] */
} rrt_clam_weights;

int rrt_clam_workspace_size(const rrt_clam_desc *desc, int64_t n_tokens, size_t *bytes);
/* Optional outputs (NULL: not wanted): a_raw [K, n_tokens] (what attention_only=True returns), attn [K, n_tokens]
 * (softmax over the bag), features [K, dim] (M), topk_idx [K, 2, k_sample] (rrt_topk_rows_f32 of attn). */
int rrt_clam_forward_f32(const rrt_clam_desc *desc, const rrt_clam_weights *w, const float *x, float *logits,
                         float *a_raw, float *attn, float *features, int64_t *topk_idx, int64_t n_tokens,
                         void *workspace, size_t workspace_bytes, void *stream);

/* ---- DSMIL head (modules/dsmil.py:96-135 MILNet with rrt=; exports added under ABI 29, no existing struct touched) ----
 * Instance stream (dsmil.py:123 i_classifier, :126 torch.max, :84-85 the sort that picks the critical instances):
 *     classes[n, j] = y_n . w[j] + b[j]   [N, C] (optional, may be NULL),
 *     cmax[j] = max_n classes[n, j]       [C]    (optional),   argmax[j] = the row that holds it   [C] int64.
 * y [N, dim], w [C, dim], b [C] or NULL.  One pass over y, fixed summation order (the same inputs give the same bits).
 * TIES: the LOWEST index wins (torch leaves it unspecified).  NaN is never selected; a column without any non-NaN value
 * selects index 0 and its cmax is NaN.  1 <= C <= 8, dim % 32 == 0, dim <= 2048, N <= 1e6, otherwise RRT_E_UNSUPPORTED.
 * workspace: rrt_instance_max_workspace_size bytes (one (max, index) record per class and 128 tokens). */
int rrt_instance_max_workspace_size(int64_t n_tokens, int32_t dim, int32_t n_classes, size_t *bytes);
int rrt_instance_max_f32(const float *y, const float *w, const float *b, float *classes, float *cmax, int64_t *argmax,
                         int64_t n_tokens, int32_t dim, int32_t n_classes, void *workspace, size_t workspace_bytes,
                         void *stream);

/* Bag stream (dsmil.py:78-94 BClassifier with nonlinear=False, passing_v=False) in ONE pass over feats [N, dim]:
 *     q_max[c] = q_w feats[argmax[c]] + q_b                       [C, Q]    (:85-86; argmax is read on the device)
 *     a_raw[n, c] = (q_w feats_n + q_b) . q_max[c] / sqrt(Q)      [N, C]    (:81, :87-88)
 *     A[:, c] = softmax_n(a_raw[:, c])                            [N, C]    (:88, the reference's layout)
 *     B[c, :] = sum_n A[n, c] feats_n                             [C, dim]  (:89)
 *     logits[o] = sum_{c, j} fcc_w[o, c, j] B[c, j] + fcc_b[o]    [C]       (:91-93, Conv1d(C, C, kernel_size = dim))
 * The scores are computed FOLDED, a_raw[n, c] = feats_n . (q_w^T q_max[c]) / sqrt(Q) + q_b . q_max[c] / sqrt(Q): Q [N, Q]
 * never exists, and feats is read once for scores and pooling (online softmax over 32-token chunks, fixed-order merge).
 * q_w [Q, dim], q_b [Q] or NULL, fcc_w [C, C, dim], fcc_b [C] or NULL.  A, B, a_raw are optional (NULL: not wanted; the
 * other outputs keep their bits).  An index outside [0, N) is clamped into the bag.  1 <= C <= 8, Q % 4 == 0, Q <= 4096,
 * dim % 32 == 0, dim <= 2048, N <= 1e6, otherwise RRT_E_UNSUPPORTED.  workspace: rrt_dsmil_pool_workspace_size bytes.
 * Not yet timed against the composition (rrt_branch_pool_f32 with y = hid_a = feats + torch ops): tools/bench_dsmil.py. */
int rrt_dsmil_pool_workspace_size(int64_t n_tokens, int32_t dim, int32_t q_dim, int32_t n_classes, size_t *bytes);
int rrt_dsmil_pool_f32(const float *feats, const int64_t *argmax, const float *q_w, const float *q_b, const float *fcc_w,
                       const float *fcc_b, float *logits, float *A, float *B, float *a_raw, int64_t n_tokens, int32_t dim,
                       int32_t q_dim, int32_t n_classes, void *workspace, size_t workspace_bytes, void *stream);

/* MILNet.forward (eval, one bag, one stream; dsmil.py:117-135): x [n_tokens, input_dim] -> Linear(input_dim, dim) + act
 * = feats (enc.compute's arithmetic, as CLAM's embedding) -> RRTEncoder (has_rrt; the reference allows rrt=None) ->
 * instance max on the ENCODER OUTPUT -> bag stream on feats, the embedding BEFORE the encoder (dsmil.py:124) -> logits.
 * Everything behind the encoder is fp32 in every compute mode: a 16-bit instance score could select another critical
 * instance, a discontinuity no tolerance covers. */
typedef struct rrt_dsmil_desc {
  rrt_encoder_desc enc;    /* has_rrt = 0: only dim (= 512 in the reference) and compute are read */
  int32_t input_dim;       /* patch feature width (multiple of 32) */
  int32_t emb_act;         /* RRT_ACT_NONE / RRT_ACT_RELU / RRT_ACT_GELU (dsmil.py:101-104) */
  int32_t has_rrt;         /* 1: the encoder sits in front of the instance classifier (dsmil.py:109, :123) */
  int32_t n_classes;       /* C, 1..8 */
  int32_t q_dim;           /* 128 in the reference (dsmil.py:65) */
} rrt_dsmil_desc;

typedef struct rrt_dsmil_weights {
  rrt_encoder_weights enc;
  const float *emb_w, *emb_b;         /* patch_to_emb.0      [dim, input_dim], [dim] */
  const float *icls_w, *icls_b;       /* i_classifier        [C, dim], [C] */
  const float *q_w, *q_b;             /* b_classifier.q      [q_dim, dim], [q_dim] */
  const float *fcc_w, *fcc_b;         /* b_classifier.fcc    [C, C, dim], [C] */
} rrt_dsmil_weights;

int rrt_dsmil_workspace_size(const rrt_dsmil_desc *desc, int64_t n_tokens, size_t *bytes);
/* logits [C] (prediction_bag); optional (NULL: not wanted): classes_max [C] (the eval-mode second output), A [n_tokens, C],
 * B [C, dim], argmax [C] int64 (the critical instances).  The indices never visit the host. */
int rrt_dsmil_forward_f32(const rrt_dsmil_desc *desc, const rrt_dsmil_weights *w, const float *x, float *logits,
                          float *classes_max, float *A, float *B, int64_t *argmax, int64_t n_tokens, void *workspace,
                          size_t workspace_bytes, void *stream);

/* ---- ABMIL / gated ABMIL / IBMIL / MeanMIL / MaxMIL heads (modules/attmil.py, attmil_ibmil.py, mean_max.py with rrt=;
 * exports added under ABI 29, no existing struct touched) ----
 * Mean pool (mean_max.py:49-52, Linear(y).mean(1); the mean commutes with the Linear, so [N, C] never exists):
 *     colmean[d] = (1/N) sum_n y[n, d]   [dim] (optional output, may be NULL; training stashes it),
 *     logits[j] = w[j] . colmean + b[j]  [C].
 * y [N, dim], w [C, dim], b [C] or NULL.  One pass over y, block partials merged in a fixed order (the same inputs give the
 * same bits); a NaN propagates.  1 <= C <= 8, dim % 32 == 0, dim <= 2048, N <= 1e6, otherwise RRT_E_UNSUPPORTED.
 * workspace: rrt_bag_mean_workspace_size bytes (one partial row per 32 rows of y, one per 64 of those). */
int rrt_bag_mean_workspace_size(int64_t n_tokens, int32_t dim, int32_t n_classes, size_t *bytes);
int rrt_bag_mean_f32(const float *y, const float *w, const float *b, float *logits, float *colmean, int64_t n_tokens,
                     int32_t dim, int32_t n_classes, void *workspace, size_t workspace_bytes, void *stream);
/* Its adjoint, from d_logits [C] and the stashed colmean [dim]: dy[n, :] = (1/N) sum_j d_logits[j] w[j] (one row, stored N
 * times: the rows are bit-identical), dW[j] = d_logits[j] colmean, db = d_logits.  Any of dy / dW / db may be NULL
 * (colmean is read for dW only).  The same limits; no workspace. */
int rrt_bag_mean_backward_f32(const float *d_logits, const float *colmean, const float *w, float *dy, float *dW, float *db,
                              int64_t n_tokens, int32_t dim, int32_t n_classes, void *stream);

/* IBMIL's deconfounder tail (attmil_ibmil.py:90-101) on a pooled bag embedding that lives in device memory:
 *     q = W_q pooled + b_q [J],  k_i = W_k conf_i + b_k [J],  a = softmax_i(k_i . q / sqrt(J)) over the K confounders,
 *     cf = sum_i a_i conf_i [V],  logits = head [pooled | cf] + head_b [C].
 * The scores are computed folded, k_i . q = conf_i . (W_k^T q) + b_k . q: k [K, J] is never formed.  pooled [dim],
 * conf [K, V], q_w [J, dim], k_w [J, V], head_w [C, dim + V]; q_b, k_b, head_b may be NULL.  Optional outputs (NULL: not
 * wanted): a [K], cf [V].  One block, fixed order.  1 <= K <= 64, dim and V multiples of 32 up to 2048 (512 in the
 * reference), J % 4 == 0, J <= 512, C >= 1, otherwise RRT_E_UNSUPPORTED. */
int rrt_deconf_head_f32(const float *pooled, const float *conf, const float *q_w, const float *q_b, const float *k_w,
                        const float *k_b, const float *head_w, const float *head_b, float *logits, float *a, float *cf,
                        int32_t dim, int32_t n_conf, int32_t conf_dim, int32_t joint_dim, int32_t n_classes, void *stream);

/* One descriptor for the five heads: x [n_tokens, input_dim] -> Linear(input_dim, dim) + act (enc.compute's arithmetic, as
 * CLAM's embedding) -> RRTEncoder (has_rrt) -> the pool -> logits [n_classes].
 *   RRT_BAGPOOL_MEAN         logits = classifier(y).mean over the bag (rrt_bag_mean_f32)
 *   RRT_BAGPOOL_MAX          logits[j] = max_n classifier(y)[n, j] (rrt_instance_max_f32: lowest index on ties, NaN never selected)
 *   RRT_BAGPOOL_ATTN         ABMIL: Linear(dim, pool_hidden) + tanh -> Linear(pool_hidden, 1) -> softmax over the bag -> classifier
 *   RRT_BAGPOOL_ATTN_GATED   the gated form: (Linear + pool_act) * (Linear + sigmoid) -> Linear(pool_hidden, 1) -> ...
 *   RRT_BAGPOOL_ATTN_DECONF  ABMIL's pooled embedding -> rrt_deconf_head_f32 (cls_w is then [n_classes, dim + deconf_v])
 * The mean and max tails are fp32 in every compute mode (a 16-bit instance score could select another instance); the
 * attention tails follow enc.compute like rrt_mil_forward_f32. */
enum { RRT_BAGPOOL_MEAN = 0, RRT_BAGPOOL_MAX = 1, RRT_BAGPOOL_ATTN = 2, RRT_BAGPOOL_ATTN_GATED = 3, RRT_BAGPOOL_ATTN_DECONF = 4 };

typedef struct rrt_bagmil_desc {
  rrt_encoder_desc enc;    /* has_rrt = 0: only dim (= 512 in the reference) and compute are read */
  int32_t input_dim;       /* patch feature width (multiple of 32) */
  int32_t emb_act;         /* RRT_ACT_NONE / RRT_ACT_RELU / RRT_ACT_GELU */
  int32_t has_rrt;         /* 1: the encoder sits between the embedding and the pool */
  int32_t n_classes;       /* MEAN / MAX: 1..8 */
  int32_t pool;            /* RRT_BAGPOOL_* */
  int32_t pool_hidden;     /* attention pools: 128 in the reference (multiple of 4) */
  int32_t pool_act;        /* ATTN_GATED: RRT_ACT_NONE / RELU / GELU / TANH of attention_a; ATTN, ATTN_DECONF: tanh whatever is set */
  int32_t deconf_k;        /* ATTN_DECONF: confounders K (1..64), their width V, the joint space J (128 in the reference) */
  int32_t deconf_v;
  int32_t deconf_j;
} rrt_bagmil_desc;

typedef struct rrt_bagmil_weights {
  rrt_encoder_weights enc;
  const float *emb_w, *emb_b;         /* the embedding Linear            [dim, input_dim], [dim] */
  const float *a_w, *a_b;             /* attention pools: first Linear   [pool_hidden, dim], [pool_hidden] or NULL */
  const float *b_w, *b_b;             /* ATTN_GATED: the gate's Linear   [pool_hidden, dim], [pool_hidden] or NULL */
  const float *c_w, *c_b;             /* attention pools: score Linear   [1, pool_hidden], [1] or NULL */
  const float *cls_w, *cls_b;         /* classifier [n_classes, dim] (ATTN_DECONF: [n_classes, dim + deconf_v]), [n_classes] or NULL */
  const float *conf;                  /* ATTN_DECONF: confounder_feat    [deconf_k, deconf_v] */
  const float *q_w, *q_b;             /* ATTN_DECONF: W_q                [deconf_j, dim], [deconf_j] */
  const float *k_w, *k_b;             /* ATTN_DECONF: W_k                [deconf_j, deconf_v], [deconf_j] */
} rrt_bagmil_weights;

int rrt_bagmil_workspace_size(const rrt_bagmil_desc *desc, int64_t n_tokens, size_t *bytes);
/* logits [n_classes]; optional (NULL: not wanted): attn [n_tokens] (attention pools: softmax over the bag, or the raw scores
 * with no_norm != 0), pooled [dim] (attention pools: the bag embedding; MEAN: the column mean), argmax [n_classes] int64
 * (MAX), deconf_a [deconf_k] and deconf_cf [deconf_v] (ATTN_DECONF).  An output the pool does not produce must be NULL
 * (RRT_E_INVALID).  Nothing visits the host. */
int rrt_bagmil_forward_f32(const rrt_bagmil_desc *desc, const rrt_bagmil_weights *w, const float *x, float *logits,
                           float *attn, int32_t no_norm, float *pooled, int64_t *argmax, float *deconf_a, float *deconf_cf,
                           int64_t n_tokens, void *workspace, size_t workspace_bytes, void *stream);

/* ---- batch-of-bags executor (BASELINE configs[4]: mixed-size bags, every bag an independent B=1 forward;
 * the reference loops `for bag in loader: model(bag)`, main.py:466-467 / :558-560) ----
 * Bags are independent units, and one bag's forward is a dependent chain of ~10 kernels that leaves
 * launch ramps, tails and store phases idle; the executor keeps `n_streams` bags in flight on its own HIP
 * streams (one workspace each, owned by the executor) so those gaps are filled by another bag's kernels.
 * rrt_executor_forward is ordered on the caller's `stream` like any other call here; the caller's stream carries the
 * first share of the bags itself and the executor's streams 1 .. n_streams-1 the others (fork: they wait for `stream`;
 * join: `stream` waits for them BEHIND its own bags -- a caller stream that only sits on the join's barrier packets is one
 * more active hardware queue, and four bag queues plus that one lose 13 % on MI355X's four pipes); a one-stream executor is
 * plain launches on `stream`, and so is a call of fewer than 8 bags on any executor (a call uses one stream per four
 * bags, at most n_streams: forking for 2-4 bags costs more than it hides -- the kernels and bits are those of the
 * executor's configured width either way); it never synchronises the host unless a
 * workspace has to grow.  One executor per host thread and device.  Set GPU_MAX_HW_QUEUES >= 8 in the
 * process environment so every stream gets its own hardware queue. */
typedef struct rrt_executor rrt_executor;
typedef struct rrt_bag {
  const float *x;      /* [n_tokens, dim] device */
  float *y;            /* [n_tokens, dim] device, != x */
  int64_t n_tokens;
} rrt_bag;
int rrt_executor_create(const rrt_encoder_desc *desc, int32_t n_streams, int64_t max_tokens,
                        rrt_executor **out);
/* The same on streams the CALLER owns (n_streams distinct hipStream_t; they are used, never destroyed): a host framework
 * hands over streams of its own pool -- rrt_mil_amd passes torch.cuda.Stream handles -- so that the process keeps ONE set of
 * streams however many executors it makes (HIP maps streams to hardware queues in creation order; streams created and
 * destroyed by executors of different widths end up sharing queues). */
int rrt_executor_create_on_streams(const rrt_encoder_desc *desc, int32_t n_streams, void *const *streams,
                                   int64_t max_tokens, rrt_executor **out);
int rrt_executor_forward(rrt_executor *ex, const rrt_encoder_weights *w, const rrt_bag *bags,
                         int32_t n_bags, void *stream);
int rrt_executor_destroy(rrt_executor *ex);

/* ---- row f2 building blocks: backward stages (assembled by rrt_encoder_backward_f32 below; parity-tested
 * on their own as well) ----
 * nn.Linear backward for Y[M,N] = X[M,K] . W[N,K]^T + b:  dX[M,K] = dY . W,  dW[N,K] = dY^T . X,
 * db[N] = column sums of dY.  Any of dX / dW / db may be NULL.  N must be a multiple of 32 when dX is
 * requested (it is the reduction length of that product). */
/* Region attention backward (rmsa.py:103-122): qkv [n_regions*P, 3*dim] as the forward stage wrote it (q scaled),
 * o = the forward output, d_o its gradient  ->  d_qkv (gradient w.r.t. the qkv linear's raw output, same layout)
 * and d_pe_w [heads, epeg_k] (NULL allowed; the conv bias gradient is exactly zero).  Head dim 64: any P (<= 208: one resident kernel; larger: a streaming four-kernel variant);
 * other multiples of 16 up to 256: any P and epeg_k <= 63 (the streaming variant at that head dim; without EPEG on P <= 128 the
 * VALU kernel below); any other multiple of 4: no EPEG and P <= 128 (a VALU kernel).  workspace:
 * rrt_region_attention_backward_workspace_size bytes. */
int rrt_region_attention_backward_workspace_size(int32_t n_regions, int32_t P, int32_t dim, int32_t heads,
                                                 int32_t epeg_k, size_t *bytes);
int rrt_region_attention_backward_f32(const float *qkv, const float *pe_w, const float *o, const float *d_o,
                                      float *d_qkv, float *d_pe_w, int32_t n_regions, int32_t P, int32_t dim,
                                      int32_t heads, int32_t epeg_k, void *workspace, size_t workspace_bytes,
                                      void *stream);
/* ---- stage entry points of the ablation kernels: one launcher each, so that a test can hold a single kernel to a reference.
 * PEG / PPEG (emb_position.py:24-82) on x [N, dim] -> y [N, dim].  w / b / dw / db: HOST arrays of three DEVICE pointers, proj
 * [dim, 1, k, kw], proj1 (5) and proj2 (3), kw = 1 when conv_1d else the kernel's side; PEG reads [0] only; b, db and any of
 * their entries may be NULL.  k odd <= 11, dim a multiple of 4.  The backward takes the stage's input x and dy, writes dx, every
 * dw and the db that are given; workspace: rrt_peg_backward_workspace_size bytes. */
int rrt_peg_f32(const float *x, const float *const *w, const float *const *b, float *y, int64_t N, int32_t dim, int32_t k,
                int32_t conv_1d, int32_t ppeg, void *stream);
int rrt_peg_backward_workspace_size(int64_t N, int32_t dim, int32_t k, int32_t ppeg, size_t *bytes);
int rrt_peg_backward_f32(const float *x, const float *dy, const float *const *w, float *dx, float *const *dw, float *const *db,
                         int64_t N, int32_t dim, int32_t k, int32_t conv_1d, int32_t ppeg, void *workspace,
                         size_t workspace_bytes, void *stream);
/* 2-D 'attn' EPEG (rmsa.py:78-79,106-108): o = softmax(S + conv2d_k(S)) V per (region, head), S = q k^T, on qkv
 * [n_regions*P, 3*dim] as the qkv linear wrote it (q scaled); pe_w [heads, k, k], k odd <= 63.  The conv bias cancels in the softmax
 * and is not an argument.  scratch: rrt_attn_scoremap_scratch_size bytes -- the forward's is 0 while a [P, P] map fits the LDS
 * (scratch may then be NULL); the backward's holds three maps per (region, head) once they no longer fit, and the per-region tap
 * partials behind them.  The backward writes d_qkv (gradient w.r.t. the qkv linear's raw output) and d_pe_w. */
int rrt_attn_scoremap_scratch_size(int32_t n_regions, int32_t P, int32_t heads, int32_t k, int32_t backward, size_t *bytes);
int rrt_attn_scoremap_f32(const float *qkv, const float *pe_w, float *o, int32_t n_regions, int32_t P, int32_t dim,
                          int32_t heads, int32_t k, void *scratch, size_t scratch_bytes, void *stream);
int rrt_attn_scoremap_backward_f32(const float *qkv, const float *pe_w, const float *d_o, float *d_qkv, float *d_pe_w,
                                   int32_t n_regions, int32_t P, int32_t dim, int32_t heads, int32_t k, void *scratch,
                                   size_t scratch_bytes, void *stream);
/* value EPEG (rmsa.py:80-85,114-129): pe [n_regions*P, dim] = depth-wise conv (k x k when two_d, else (k, 1)) over the v columns of
 * qkv laid out as an s x s image per region (P = s*s), image channel c reading v column (c % heads) * (dim / heads) + c / heads;
 * w [dim, 1, k, kw], bias [dim] or NULL.  The backward ADDS the conv's dv into the v columns of d_qkv (q and k columns untouched),
 * writes d_w and, when given, d_b; vsub [n_regions*P, dim] (or NULL) is subtracted from the v columns first ('value_bf' keeps
 * v + pe in qkv). */
int rrt_value_pe_f32(const float *qkv, const float *w, const float *bias, float *pe, int32_t n_regions, int32_t P, int32_t s,
                     int32_t dim, int32_t heads, int32_t k, int32_t two_d, void *stream);
int rrt_value_pe_backward_f32(const float *d_pe, const float *qkv, const float *vsub, const float *w, float *d_qkv, float *d_w,
                              float *d_b, int32_t n_regions, int32_t P, int32_t s, int32_t dim, int32_t heads, int32_t k,
                              int32_t two_d, void *stream);
/* LayerNorm backward (eps 1e-5): dx [L, dim] = d/dx of LN(x) . dy (+ add, the residual branch's gradient,
 * optional); dgamma_dbeta [2, dim].  g != NULL: dy is region-major padded [H*H, dim] (the qkv-linear backward's
 * output) and token t reads its slot -- the adjoint of zero-pad + region_partition.  workspace: 512*2*dim floats. */
int rrt_layernorm_backward_f32(const float *dy, const float *x, const float *gamma, const float *add,
                               float *dx, float *dgamma_dbeta, int64_t L, int32_t dim, const rrt_grid *g,
                               void *workspace, size_t workspace_bytes, void *stream);
/* Fixed-order sum of S partial vectors: out[i] = sum_s part[s * n + i] (the parameter-gradient reductions of the backward:
 * LayerNorm's d gamma | d beta, the EPEG taps, CR-MSA's norm / phi rows, the weight gradients' split-K chunks).
 * out_tr != NULL: out takes only [0, split) and the tail [tr_k, tr_dim] (n - split = tr_k * tr_dim, split % 4 == 0) leaves
 * transposed in out_tr [tr_dim, tr_k].  deferred = 0: the stage's own launch (256 elements per block); 1: through the
 * backward's job list and its one launch at the end of the pass (a block per 128-byte line of every partial), the job queued
 * `copies` (1 .. 16) times -- copy c reads the same partials and writes out + c * n (out_tr + c * tr_dim * tr_k).
 * Bit-reproducible in either form; the two forms sum in different orders. */
int rrt_reduce_partials_f32(const float *part, float *out, float *out_tr, int32_t S, int64_t n, int64_t split,
                            int32_t tr_dim, int32_t tr_k, int32_t deferred, int32_t copies, void *stream);
int rrt_linear_backward_workspace_size(int64_t M, int32_t N, int32_t K, size_t *bytes);
int rrt_linear_backward_f32(const float *dY, const float *X, const float *W, float *dX, float *dW,
                            float *db, int64_t M, int32_t N, int32_t K, int32_t compute,
                            void *workspace, size_t workspace_bytes, void *stream);

/* Stage entries for tests: the element-wise passes of the training step (csrc/ln_bwd.hip) and the batched weight transpose
 * (csrc/linear_bwd.hip), one launcher each, which only the whole-encoder entries reached before (exports added under ABI 29,
 * no existing struct or signature touched; tests/test_train_blocks_matrix.py, tests/test_train_blocks_grid_cpu.py).
 * Dropout: threshold, scale 1/(1-p) and seed are derived from (drop_p, drop_seed, drop_layer) exactly as
 * rrt_encoder_forward_train_f32 / rrt_encoder_backward_f32 derive them (drop_layer: any non-negative tag, e.g. the R-MSA layer
 * index, 100 for CR-MSA); element i is kept iff hash(seed, layer, i) >= p * 2^32.  drop_p = 0: no mask.  Every entry checks
 * its arguments before it launches: RRT_E_INVALID on NULL / non-positive / inconsistent ones, RRT_E_UNSUPPORTED as noted.
 *   act_forward     h[i] = act(hpre[i]), then the mask (index i) and the scale 1/(1-p).  act = RRT_ACT_GELU (exact, erf) or
 *                   RRT_ACT_RELU, n % 4 == 0 (else RRT_E_UNSUPPORTED).
 *   act_backward    in place: dh[i] = mask(dh[i]) * scale * act'(hpre[i]); ReLU's derivative at +-0 is 0.  dh != hpre.
 *   partition_rows  dst [H*H, dim] region-major <- src [g->L, dim] token order, pad slots 0 (region_partition of a gradient),
 *                   times `scale` (a branch multiplier, >= 0) and, with drop_p > 0, the mask indexed by PADDED SLOT * dim +
 *                   column and 1/(1-p).  dim % 4 == 0 (else RRT_E_UNSUPPORTED), H*H <= 2^24, src != dst.
 *   drop_mask       dst[i] = keep(i) ? src[i] * scale / (1-p) : 0 for any n <= 2^31 - 1, no alignment assumed; src == dst runs
 *                   the in-place form (which launches nothing when drop_p == 0 and scale == 1), else the copying form.
 *   transpose_batch out[j] [C[j], R[j]] = in[j] [R[j], C[j]]^T for n_jobs matrices in ONE launch; in, out, R, C are HOST
 *                   arrays of n_jobs entries.  n_jobs <= 2 * RRT_MAX_RMSA_LAYERS + 2 (else RRT_E_UNSUPPORTED). */
int rrt_debug_act_forward_f32(const float *hpre, float *h, int64_t n, int32_t act, float drop_p, uint64_t drop_seed,
                              int32_t drop_layer, void *stream);
int rrt_debug_act_backward_f32(float *dh, const float *hpre, int64_t n, int32_t act, float drop_p, uint64_t drop_seed,
                               int32_t drop_layer, void *stream);
int rrt_debug_partition_rows_f32(const float *src, float *dst, int32_t dim, const rrt_grid *g, float drop_p,
                                 uint64_t drop_seed, int32_t drop_layer, float scale, void *stream);
int rrt_debug_drop_mask_f32(const float *src, float *dst, int64_t n, float drop_p, uint64_t drop_seed, int32_t drop_layer,
                            float scale, void *stream);
int rrt_debug_transpose_batch_f32(const float *const *in, float *const *out, const int32_t *R, const int32_t *C,
                                  int32_t n_jobs, void *stream);

/* ---- row f2: training.  Forward that stashes what the backward needs, and the backward itself ----
 * Supported: the default path (1-D 'attn' EPEG R-MSA layers, CR-MSA with the phi matrix or the MLP phi,
 * all_shortcut), an R-MSA head dim that is a multiple of 16 up to 256 (any other multiple of 4 without EPEG on regions of
 * <= 128 tokens; any multiple of 4 in CR-MSA's inner attention), bags of any size, dim <= 1024, F32 compute.  Anything
 * else: RRT_E_UNSUPPORTED.
 * drop_p / drop_seed: the train-mode proj_drop of every InnerAttention (rmsa.py:70,132; p = drop_out): a stateless
 * mask, element kept iff hash(seed, layer, index) >= p * 2^32, kept values scaled by 1/(1-p); the backward call
 * must receive the same (drop_p, drop_seed) as its forward.  drop_p = 0: no dropout.
 * branch_scale (HOST pointer, may be NULL = all ones): stochastic depth, TransLayer.drop_path (rrt.py:102,125,129;
 * timm's DropPath at batch size 1 keeps or drops a whole residual branch): 2 * (RRT_MAX_RMSA_LAYERS + 1) multipliers,
 * first the attention branches (index n_rmsa_layers = CR-MSA's), then the FFN branches in the same order; each is
 * 1 (drop_path = 0), 1 / keep_prob (kept) or 0 (dropped).  The caller draws them; forward and backward get the same.
 * Gradients mirror the parameters: norm = [2, dim] (d gamma then d beta); pe bias gradients are exactly zero and
 * are not written.  NULL gradient pointers are not allowed for parameters the model has. */
typedef struct rrt_attn_grads {
  float *norm;                 /* [2, dim] */
  float *qkv_w, *qkv_b;        /* qkv_b NULL when qkv_bias = False */
  float *proj_w, *proj_b;
  float *pe_w;                 /* [heads, epeg_k] or NULL (epeg_2d: [heads, k, k]; epeg_type value_*: [dim, k] / [dim, k, k]) */
  float *pe_b;                 /* epeg_type value_* with a conv bias: [dim]; NULL otherwise (the 'attn' conv bias has an
                                  exactly zero gradient: it cancels in the softmax) */
  float *norm2;                /* ffn = 1: [2, dim] */
  float *fc1_w, *fc1_b;        /* ffn = 1: [ffn_hidden, dim], [ffn_hidden] */
  float *fc2_w, *fc2_b;        /* ffn = 1: [dim, ffn_hidden], [dim] */
} rrt_attn_grads;
typedef struct rrt_encoder_grads {
  rrt_attn_grads rmsa[RRT_MAX_RMSA_LAYERS];
  rrt_attn_grads crmsa;
  float *phi;                  /* [dim, crmsa_k]                              (crmsa_mlp = 0) */
  float *phi0_w, *phi2_w;      /* [dim/4, dim], [crmsa_k, dim/4]              (crmsa_mlp = 1) */
  float *norm;                 /* [2, dim] final LayerNorm */
  float *pos_w[3], *pos_b[3];  /* pos_embedding.proj / proj1 / proj2 (pos != none) */
} rrt_encoder_grads;

int rrt_encoder_train_sizes(const rrt_encoder_desc *desc, int64_t n_tokens, size_t *stash_bytes,
                            size_t *backward_workspace_bytes);
/* y = RRTEncoder(x) (eval-equivalent arithmetic), intermediates kept in the caller-owned stash */
int rrt_encoder_forward_train_f32(const rrt_encoder_desc *desc, const rrt_encoder_weights *w, const float *x,
                                  float *y, int64_t n_tokens, void *stash, size_t stash_bytes,
                                  float drop_p, uint64_t drop_seed, const float *branch_scale, void *stream);
/* given dy = dL/dy: every parameter gradient and (optional) dx = dL/dx.  x and the stash are those of the forward. */
int rrt_encoder_backward_f32(const rrt_encoder_desc *desc, const rrt_encoder_weights *w, const float *x,
                             const float *dy, const void *stash, size_t stash_bytes,
                             const rrt_encoder_grads *grads, float *dx, int64_t n_tokens, void *workspace,
                             size_t workspace_bytes, float drop_p, uint64_t drop_seed,
                             const float *branch_scale, void *stream);

/* The same pair for the part of an encoder BEHIND its attention layers (CR-MSA, all_shortcut, the final LayerNorm), for callers
 * that run the attention layers themselves (the Nystrom ablations' training path; exports added under ABI 29, the pair above
 * and its bits unchanged).  desc must have n_rmsa_layers = 0 and pos none (else RRT_E_UNSUPPORTED); sizes are
 * rrt_encoder_train_sizes' for that desc.  x1 [n_tokens, dim] is the attention layers' output, x0 what all_shortcut adds (the
 * encoder's ORIGINAL input; read, and d_x0 written, only when desc->all_shortcut, and then neither may be NULL).  backward
 * writes d_x1 (or skips it when NULL) without the shortcut's share, which goes to d_x0.  CR-MSA's stochastic-depth multiplier
 * is branch_scale[0] (its layer index is n_rmsa_layers = 0). */
int rrt_encoder_tail_forward_train_f32(const rrt_encoder_desc *desc, const rrt_encoder_weights *w, const float *x1,
                                       const float *x0, float *y, int64_t n_tokens, void *stash, size_t stash_bytes,
                                       float drop_p, uint64_t drop_seed, const float *branch_scale, void *stream);
int rrt_encoder_tail_backward_f32(const rrt_encoder_desc *desc, const rrt_encoder_weights *w, const float *x1, const float *dy,
                                  const void *stash, size_t stash_bytes, const rrt_encoder_grads *grads, float *d_x1,
                                  float *d_x0, int64_t n_tokens, void *workspace, size_t workspace_bytes, float drop_p,
                                  uint64_t drop_seed, const float *branch_scale, void *stream);

/* ---- Nystrom attention and the TransMIL baseline (modules/nystrom_attention.py:67-149, modules/transmil.py:26-125; exports
 * added under ABI 29, no existing struct touched).  Inference, exact fp32 on the fp32 matrix cores, no atomics: the same inputs
 * give the same bits.  There is no mask argument (the reference's mask branch names undefined variables).
 * Supported: dim_head = 64, num_landmarks = 256, residual_conv_kernel odd <= 63, pinv_iterations 1..16, heads 1..16,
 * dim % 32 == 0, dim <= 1024, n <= 1e6; otherwise RRT_E_UNSUPPORTED with the field's name in rrt_strerror. */
typedef struct rrt_nystrom_desc {
  int32_t dim;
  int32_t heads;
  int32_t dim_head;
  int32_t num_landmarks;
  int32_t pinv_iterations;
  int32_t residual;              /* 1: + the depth-wise conv of v along the tokens (res_conv) */
  int32_t residual_conv_kernel;
} rrt_nystrom_desc;

/* to_qkv.weight [3 * heads * dim_head, dim] (no bias), to_out.0.weight [dim, heads * dim_head], to_out.0.bias [dim],
 * res_conv.weight [heads, 1, k, 1] (read only when residual != 0) */
typedef struct rrt_nystrom_weights {
  const float *qkv_w;
  const float *out_w, *out_b;
  const float *conv_w;
} rrt_nystrom_weights;

int rrt_nystrom_workspace_size(const rrt_nystrom_desc *desc, int64_t n, size_t *bytes);
/* NystromAttention.forward: x [n, dim] (already normalised by the caller's LayerNorm) -> y [n, dim]; the caller's residual
 * is NOT included.  np = n rounded up to a multiple of 256; the np - n zero rows go in FRONT of x and take part in the
 * landmarks, in both softmaxes over the keys and in the conv, as in the reference. */
int rrt_nystrom_attention_f32(const rrt_nystrom_desc *desc, const rrt_nystrom_weights *w, const float *x, float *y,
                              int64_t n, void *workspace, size_t workspace_bytes, void *stream);

/* Stage entry points, one per kernel.  n_padded = np, a positive multiple of 256 (l = np / 256).
 * qkv [np, 3 * heads * 64]: the qkv linear's output, q columns already scaled by 64^-0.5, front pad rows zero.
 *  landmarks     : ql, kl [heads, 256, 64] = means of l consecutive rows of q and of k (divisor always l);
 *  landmark_sim  : a2 [heads, 256, 256] = softmax(ql kl^T);
 *  landmark_attn : av [heads, 256, 64] = softmax(ql k^T) v over all np keys (chunks of keys with an online softmax, the
 *                  chunk records merged in chunk order);
 *  pinv          : z [heads, 256, 256] = `iterations` steps of z <- 1/4 z (13 I - a2 z (15 I - a2 z (7 I - a2 z))) from
 *                  z0 = a2^T / (max row abs sum * max column abs sum), both maxima over ALL heads;
 *  zav           : wz [heads, 256, 64] = z av;
 *  output        : o [np, heads * 64] = softmax(q kl^T) wz + conv_k(v) (conv_w [heads, conv_k] or NULL = no conv), heads merged. */
int rrt_nystrom_landmarks_f32(const float *qkv, float *ql, float *kl, int64_t n_padded, int32_t heads, void *stream);
int rrt_nystrom_landmark_sim_f32(const float *ql, const float *kl, float *a2, int32_t heads, void *stream);
int rrt_nystrom_landmark_attn_workspace_size(int64_t n_padded, int32_t heads, size_t *bytes);
int rrt_nystrom_landmark_attn_f32(const float *qkv, const float *ql, float *av, int64_t n_padded, int32_t heads,
                                  void *workspace, size_t workspace_bytes, void *stream);
int rrt_nystrom_pinv_workspace_size(int32_t heads, size_t *bytes);
int rrt_nystrom_pinv_f32(const float *a2, float *z, int32_t heads, int32_t iterations, void *workspace,
                         size_t workspace_bytes, void *stream);
int rrt_nystrom_zav_f32(const float *z, const float *av, float *wz, int32_t heads, void *stream);
int rrt_nystrom_output_f32(const float *qkv, const float *kl, const float *wz, const float *conv_w, float *o,
                           int64_t n_padded, int32_t heads, int32_t conv_k, void *stream);

/* ---- Batched Nystrom attention (exports added under ABI 29; nothing above changes).  b sequences of n tokens each in ONE launch
 * per stage -- no host loop over b.  Every layout above gains a leading b: qkv [b, np, 3 * heads * 64] (each item's np - n zero
 * rows in FRONT of that item), ql / kl / av / wz [b, heads, 256, 64], a2 / z [b, heads, 256, 256], o [b, np, heads * 64].  The
 * conv runs along each item's own padded sequence.  The pseudo-inverse's initial scale is ONE scalar, max row abs sum * max
 * column abs sum over all b * heads matrices of a2 (the reference's torch.max over the whole batch), reduced without atomics in
 * a fixed order.  Envelope: the single-sequence one plus 1 <= b <= 4096.  Two calls give the same bits, and with b = 1 every
 * entry gives the bits of its single-sequence counterpart.
 * attention_batched: x [b, n, dim] -> y [b, n, dim]. */
int rrt_nystrom_batched_workspace_size(const rrt_nystrom_desc *desc, int64_t b, int64_t n, size_t *bytes);
int rrt_nystrom_attention_batched_f32(const rrt_nystrom_desc *desc, const rrt_nystrom_weights *w, const float *x, float *y,
                                      int64_t b, int64_t n, void *workspace, size_t workspace_bytes, void *stream);
int rrt_nystrom_landmarks_batched_f32(const float *qkv, float *ql, float *kl, int64_t b, int64_t n_padded, int32_t heads,
                                      void *stream);
int rrt_nystrom_landmark_sim_batched_f32(const float *ql, const float *kl, float *a2, int64_t b, int32_t heads, void *stream);
int rrt_nystrom_landmark_attn_batched_workspace_size(int64_t b, int64_t n_padded, int32_t heads, size_t *bytes);
int rrt_nystrom_landmark_attn_batched_f32(const float *qkv, const float *ql, float *av, int64_t b, int64_t n_padded,
                                          int32_t heads, void *workspace, size_t workspace_bytes, void *stream);
int rrt_nystrom_pinv_batched_workspace_size(int64_t b, int32_t heads, size_t *bytes);
int rrt_nystrom_pinv_batched_f32(const float *a2, float *z, int64_t b, int32_t heads, int32_t iterations, void *workspace,
                                 size_t workspace_bytes, void *stream);
int rrt_nystrom_zav_batched_f32(const float *z, const float *av, float *wz, int64_t b, int32_t heads, void *stream);
int rrt_nystrom_output_batched_f32(const float *qkv, const float *kl, const float *wz, const float *conv_w, float *o, int64_t b,
                                   int64_t n_padded, int32_t heads, int32_t conv_k, void *stream);

/* ---- The reference's Nystrom ablations of RRTEncoder (modules/rrt.py:49-58 `--attn ntrans`, modules/rmsa.py:167-173
 * `--region_attn ntrans`; exports added under ABI 29).  One call per bag, inference, exact fp32 (desc->compute other than
 * RRT_COMPUTE_F32 is RRT_E_UNSUPPORTED).  rrt_encoder_desc describes everything but the n_rmsa_layers attention layers, whose
 * parameters ride in the rrt_attn_weights slots: norm_* the TransLayer's LayerNorm, qkv_w = to_qkv.weight (qkv_b NULL),
 * proj_w / proj_b = to_out.0.*, pe_w = res_conv.weight [heads, k], norm2 / fc* the optional FFN.  nys->attn.dim must be
 * desc->dim and attn.heads * attn.dim_head == dim; the epeg* fields are ignored.
 *  RRT_NYSTROM_BAG     : each layer is x + NystromAttention(LN(x)) over the whole bag (b = 1);
 *  RRT_NYSTROM_REGIONS : LN(x), zero rows appended to H * H, partitioned by rrt_region_grid into R regions of P tokens, the
 *                        batched attention with b = R, n = P (ONE pseudo-inverse scale over all regions and heads),
 *                        un-partitioned, the appended rows dropped, + x.
 * PEG / PPEG, CR-MSA, all_shortcut and the final LayerNorm are those of rrt_encoder_forward_f32. */
enum { RRT_NYSTROM_BAG = 1, RRT_NYSTROM_REGIONS = 2 };
typedef struct rrt_encoder_nystrom_desc {
  int32_t mode;
  rrt_nystrom_desc attn;
} rrt_encoder_nystrom_desc;
int rrt_encoder_nystrom_workspace_size(const rrt_encoder_desc *desc, const rrt_encoder_nystrom_desc *nys, int64_t n_tokens,
                                       size_t *bytes);
int rrt_encoder_nystrom_forward_f32(const rrt_encoder_desc *desc, const rrt_encoder_nystrom_desc *nys,
                                    const rrt_encoder_weights *w, const float *x, float *y, int64_t n_tokens, void *workspace,
                                    size_t workspace_bytes, void *stream);

/* ---- Nystrom attention, training (exports added under ABI 29, no existing struct or signature touched).  Exact fp32 on the
 * fp32 matrix cores, no atomics: two runs give the same bits.  The same envelope as the forward above.
 *
 * forward_train: y is bit-identical to rrt_nystrom_attention_f32; what the backward reads (qkv, the landmarks, a2, z, av, wz,
 * o and the row log-sum-exp of ql k^T) stays in the caller-owned stash of rrt_nystrom_train_sizes' stash_bytes.
 * backward: dy [n, dim] -> the parameter gradients (WRITTEN, not accumulated; conv_w [heads, k] is unused when
 * residual = 0) and, when dx is not NULL, dx [n, dim].  x and w are the forward's. */
typedef struct rrt_nystrom_grads {
  float *qkv_w;
  float *out_w, *out_b;
  float *conv_w;
} rrt_nystrom_grads;

int rrt_nystrom_train_sizes(const rrt_nystrom_desc *desc, int64_t n, size_t *stash_bytes, size_t *backward_workspace_bytes);
int rrt_nystrom_attention_forward_train_f32(const rrt_nystrom_desc *desc, const rrt_nystrom_weights *w, const float *x,
                                            float *y, int64_t n, void *stash, size_t stash_bytes, void *stream);
int rrt_nystrom_attention_backward_f32(const rrt_nystrom_desc *desc, const rrt_nystrom_weights *w, const float *x,
                                       const float *dy, const void *stash, size_t stash_bytes,
                                       const rrt_nystrom_grads *grads, float *dx, int64_t n, void *workspace,
                                       size_t workspace_bytes, void *stream);

/* Backward stage entry points, one per kernel group (layouts as the forward stages; d_qkv is the gradient of the qkv linear's
 * output with the q columns still scaled, i.e. before the 64^-0.5 of the epilogue is applied to it).
 *  output_backward        : qkv, kl, wz, conv_w (or NULL), d_o [np, heads * 64] -> d_qkv (q and v thirds written, k third
 *                           zeroed), d_kl, d_wz [heads, 256, 64], d_conv_w [heads, conv_k] (untouched when conv_w is NULL);
 *  zav_backward           : z, av, d_wz -> d_z [heads, 256, 256], d_av [heads, 256, 64];
 *  landmark_attn_backward : qkv, ql, d_av -> d_ql (written); ADDS dk, dv into the k and v thirds of d_qkv, q third untouched;
 *  pinv_sim_backward      : ql, kl, d_z -> d_ql, d_kl (written): the gradient of pinv(softmax(ql kl^T)), including the part
 *                           through the all-heads scale of z0 (its largest-column-sum factor; the largest-row-sum factor
 *                           has no gradient behind a softmax);
 *  landmarks_backward     : ADDS d_ql[j] / l and d_kl[j] / l into the q and k thirds of the l rows of landmark j. */
int rrt_nystrom_output_backward_workspace_size(int64_t n_padded, int32_t heads, size_t *bytes);
int rrt_nystrom_output_backward_f32(const float *qkv, const float *kl, const float *wz, const float *conv_w, const float *d_o,
                                    float *d_qkv, float *d_kl, float *d_wz, float *d_conv_w, int64_t n_padded, int32_t heads,
                                    int32_t conv_k, void *workspace, size_t workspace_bytes, void *stream);
int rrt_nystrom_zav_backward_f32(const float *z, const float *av, const float *d_wz, float *d_z, float *d_av, int32_t heads,
                                 void *stream);
int rrt_nystrom_landmark_attn_backward_workspace_size(int64_t n_padded, int32_t heads, size_t *bytes);
int rrt_nystrom_landmark_attn_backward_f32(const float *qkv, const float *ql, const float *d_av, float *d_qkv, float *d_ql,
                                           int64_t n_padded, int32_t heads, void *workspace, size_t workspace_bytes,
                                           void *stream);
int rrt_nystrom_pinv_sim_backward_workspace_size(int32_t heads, int32_t iterations, size_t *bytes);
int rrt_nystrom_pinv_sim_backward_f32(const float *ql, const float *kl, const float *d_z, float *d_ql, float *d_kl,
                                      int32_t heads, int32_t iterations, void *workspace, size_t workspace_bytes,
                                      void *stream);
int rrt_nystrom_landmarks_backward_f32(const float *d_ql, const float *d_kl, float *d_qkv, int64_t n_padded, int32_t heads,
                                       void *stream);

/* ---- Batched Nystrom attention, training (exports added under ABI 29; nothing above changes).  The reference's autograd on a
 * (b, n, dim) batch, b sequences per launch: exact fp32 on the fp32 matrix cores, no atomics, every sum in a fixed order (the
 * parameter gradients are summed over the items in item order), two calls give the same bits.  Layouts are those of the
 * batched forward stages above (a leading b; each item's np - n zero rows in FRONT of that item).  What a batch changes:
 *  - the pseudo-inverse's den is ONE scalar over all b * heads matrices, so d den is the sum of <d_z, the tangent of z along
 *    the scale of z0> over every item and head, and it goes to the columns that attain the largest column sum ANYWHERE in
 *    the batch, shared evenly among columns whose sums are equal bit for bit, across items too;
 *  - the stencil's adjoint and d_conv_w run along each item's own padded sequence; d_conv_w is summed over the items;
 *  - d_o's pad rows are zero and d_qkv's pad rows are dropped in front of the qkv linear's backward.
 * Envelope: the single-sequence one plus 1 <= b <= 2048 (b * heads stays a valid grid dimension) and b * n <= 4e6; beyond
 * it the size functions and every entry return RRT_E_UNSUPPORTED naming b.  A short stash or workspace is RRT_E_WORKSPACE.
 * With b = 1 every entry takes the single-sequence code path and gives the bits of its single-sequence counterpart.
 * batched_train_sizes: the stash is the batched forward's workspace kept whole plus the row log-sum-exp [b, heads, 256]; the
 *   backward's workspace holds (pinv_iterations + 10) matrices per (item, head) -- 2 GiB at b = 64, 8 heads, 6 iterations.
 * forward_train: x [b, n, dim] -> y [b, n, dim], bit-identical to rrt_nystrom_attention_batched_f32.
 * backward: dy [b, n, dim] -> grads (WRITTEN, not accumulated) and, unless NULL, dx [b, n, dim].
 * The stage entries are the single-sequence ones above with b in front of the sizes. */
int rrt_nystrom_batched_train_sizes(const rrt_nystrom_desc *desc, int64_t b, int64_t n, size_t *stash_bytes,
                                    size_t *backward_workspace_bytes);
int rrt_nystrom_attention_batched_forward_train_f32(const rrt_nystrom_desc *desc, const rrt_nystrom_weights *w, const float *x,
                                                    float *y, int64_t b, int64_t n, void *stash, size_t stash_bytes,
                                                    void *stream);
int rrt_nystrom_attention_batched_backward_f32(const rrt_nystrom_desc *desc, const rrt_nystrom_weights *w, const float *x,
                                               const float *dy, const void *stash, size_t stash_bytes,
                                               const rrt_nystrom_grads *grads, float *dx, int64_t b, int64_t n, void *workspace,
                                               size_t workspace_bytes, void *stream);
int rrt_nystrom_output_batched_backward_workspace_size(int64_t b, int64_t n_padded, int32_t heads, size_t *bytes);
int rrt_nystrom_output_batched_backward_f32(const float *qkv, const float *kl, const float *wz, const float *conv_w,
                                            const float *d_o, float *d_qkv, float *d_kl, float *d_wz, float *d_conv_w, int64_t b,
                                            int64_t n_padded, int32_t heads, int32_t conv_k, void *workspace,
                                            size_t workspace_bytes, void *stream);
int rrt_nystrom_zav_batched_backward_f32(const float *z, const float *av, const float *d_wz, float *d_z, float *d_av, int64_t b,
                                         int32_t heads, void *stream);
int rrt_nystrom_landmark_attn_batched_backward_workspace_size(int64_t b, int64_t n_padded, int32_t heads, size_t *bytes);
int rrt_nystrom_landmark_attn_batched_backward_f32(const float *qkv, const float *ql, const float *d_av, float *d_qkv,
                                                   float *d_ql, int64_t b, int64_t n_padded, int32_t heads, void *workspace,
                                                   size_t workspace_bytes, void *stream);
int rrt_nystrom_pinv_sim_batched_backward_workspace_size(int64_t b, int32_t heads, int32_t iterations, size_t *bytes);
int rrt_nystrom_pinv_sim_batched_backward_f32(const float *ql, const float *kl, const float *d_z, float *d_ql, float *d_kl,
                                              int64_t b, int32_t heads, int32_t iterations, void *workspace,
                                              size_t workspace_bytes, void *stream);
int rrt_nystrom_landmarks_batched_backward_f32(const float *d_ql, const float *d_kl, float *d_qkv, int64_t b, int64_t n_padded,
                                               int32_t heads, void *stream);

/* TransMIL's PPEG (transmil.py:47-61): x, y [1 + side * side, dim]; row 0 (the cls token) passes through, the other rows as
 * a side x side image become x + conv7(x) + conv5(x) + conv3(x), depth-wise with zero borders.  The side is EXACTLY the
 * caller's (rrt_peg_f32 derives it from the row count, wraps, and lifts sides below 7 to 7).  w / b: HOST arrays of three
 * DEVICE pointers proj [dim, 1, 7, 7], proj1 (5), proj2 (3); b or its entries may be NULL.  dim % 4 == 0, side <= 1000. */
int rrt_ppeg_side_f32(const float *x, const float *const *w, const float *const *b, float *y, int32_t side, int32_t dim,
                      void *stream);

/* TransMIL.forward (eval, one bag): _fc1 Linear(input_dim, dim) + act -> wrap to H * H rows (H = ceil(sqrt(N))) ->
 * cls token in front -> x + Nystrom(LN(x)) -> PPEG -> x + Nystrom(LN(x)) -> LN, row 0 -> _fc2. */
typedef struct rrt_transmil_desc {
  int32_t input_dim;       /* patch feature width (multiple of 32) */
  int32_t n_classes;       /* 1..64 */
  int32_t act;             /* RRT_ACT_RELU / RRT_ACT_GELU / RRT_ACT_NONE */
  rrt_nystrom_desc attn;   /* both layers; attn.dim is the model width (512 in the reference) */
} rrt_transmil_desc;

typedef struct rrt_transmil_layer_weights {
  const float *norm_w, *norm_b;   /* layer{1,2}.norm */
  rrt_nystrom_weights attn;        /* layer{1,2}.attn */
} rrt_transmil_layer_weights;

typedef struct rrt_transmil_weights {
  const float *fc1_w, *fc1_b;      /* _fc1.0 [dim, input_dim], [dim] */
  const float *cls_token;          /* [dim] */
  rrt_transmil_layer_weights layer[2];
  const float *pos_w[3], *pos_b[3];/* pos_layer.proj / proj1 / proj2 */
  const float *norm_w, *norm_b;    /* norm */
  const float *fc2_w, *fc2_b;      /* _fc2 [n_classes, dim], [n_classes] */
} rrt_transmil_weights;

int rrt_transmil_workspace_size(const rrt_transmil_desc *desc, int64_t n_tokens, size_t *bytes);
/* x [n_tokens, input_dim] -> logits [n_classes].  feat (optional, [1 + H * H, dim]): the rows before the last LayerNorm. */
int rrt_transmil_forward_f32(const rrt_transmil_desc *desc, const rrt_transmil_weights *w, const float *x, float *logits,
                             float *feat, int64_t n_tokens, void *workspace, size_t workspace_bytes, void *stream);

/* ---- Attention maps: one query row of the Nystrom-approximated attention matrix (modules/nystrom_attention.py:143-147, the
 * return_attn branch; exports added under ABI 29, no existing struct or signature touched).  Inference, exact fp32 on the
 * fp32 matrix cores, no atomics, fixed summation order: the same inputs give the same bits.  Per head, for query row t of the
 * unpadded sequence (pad = np - n zero rows in front):
 *   a1 = softmax(q[pad + t] kl^T) [256];  r = a1 z [256];  lse3_i = logsumexp_j(ql_i . k_j) over ALL np keys;
 *   attn[j] = sum_i r_i exp(ql_i . k_j - lse3_i),  j = 0 .. np - 1
 * softmax(ql k^T) [256, np] is never written.  The row is NOT a probability vector: the pad keys keep their share (the n
 * real columns do not sum to 1) and entries can be negative (z is an iterated pseudo-inverse).  The reference itself reads
 * row 0 of the PADDED sequence, a zero pad row whenever n % 256 != 0; here the row is always pad + t.
 *
 * attn_row (stage): qkv, ql, kl, z as the stage entry points above leave them, lse3 [heads, 256], row_padded in
 *   [0, n_padded) -> r [heads, 256] and attn [heads, n_padded] (ALL padded columns: sum_j attn[h, j] = sum_i r[h, i]).
 * attention_row: rrt_nystrom_attention_f32 plus row `row` in [0, n) -> attn [heads, n] (the n real columns); y has the bits
 *   of rrt_nystrom_attention_f32.  Its workspace is rrt_nystrom_attention_row_workspace_size's.
 * transmil_forward_attn: rrt_transmil_forward_f32 plus attn1 / attn2 [heads, 1 + H * H] (either may be NULL): the cls
 *   token's row in layer 1 / layer 2, the cls column (0) and the wrapped rows included; logits and feat have the bits of
 *   rrt_transmil_forward_f32.  Its workspace is rrt_transmil_attn_workspace_size's.
 * A row outside its range is RRT_E_UNSUPPORTED with "row" in rrt_strerror. */
int rrt_nystrom_attn_row_f32(const float *qkv, const float *ql, const float *kl, const float *z, const float *lse3, float *r,
                             float *attn, int64_t row_padded, int64_t n_padded, int32_t heads, void *stream);
int rrt_nystrom_attention_row_workspace_size(const rrt_nystrom_desc *desc, int64_t n, size_t *bytes);
int rrt_nystrom_attention_row_f32(const rrt_nystrom_desc *desc, const rrt_nystrom_weights *w, const float *x, float *y,
                                  int64_t row, float *attn, int64_t n, void *workspace, size_t workspace_bytes, void *stream);
int rrt_transmil_attn_workspace_size(const rrt_transmil_desc *desc, int64_t n_tokens, size_t *bytes);
int rrt_transmil_forward_attn_f32(const rrt_transmil_desc *desc, const rrt_transmil_weights *w, const float *x, float *logits,
                                  float *feat, float *attn1, float *attn2, int64_t n_tokens, void *workspace,
                                  size_t workspace_bytes, void *stream);

/* ---- TransMIL, training: one forward call and one backward call for the whole model (exports added under ABI 29, no existing
 * struct or signature touched).  Exact fp32, no atomics, no state in the library, every reduction in a fixed order: two runs
 * give the same bits.  The envelope of rrt_transmil_forward_f32; the conventions of rrt_encoder_forward_train_f32 /
 * rrt_encoder_backward_f32: caller-owned stash and workspace of rrt_transmil_train_sizes' sizes (a short one is
 * RRT_E_WORKSPACE), stream-ordered, re-entrant, every argument checked before anything is launched.
 *
 * forward_train: x [n_tokens, input_dim] -> logits [n_classes] (the loss stays with the caller); what the backward reads stays
 *   in the stash: _fc1's pre-activation (when there is an activation), the rows before and after both LayerNorms, both
 *   attentions' stashes, and the one row the head sees.  After layer 2 only row 0 (the cls token) is read: the mask, the
 *   residual, the last LayerNorm and _fc2 run on that one row.
 * backward: d_logits [n_classes] -> every parameter gradient (WRITTEN, not accumulated; grads mirrors rrt_transmil_weights,
 *   one float* per parameter, same shapes; attn.conv_w may be NULL when residual = 0) and, unless dx is NULL, dx
 *   [n_tokens, input_dim] (NULL skips _fc1's dX product).  x, w and the three dropout arguments are the forward's.
 * Dropout: the stateless mask of rrt_debug_drop_mask_f32 (kept iff hash(seed, index) >= p * 2^32, kept values scaled by
 *   1 / (1 - p)), element index = row * dim + column of the masked tensor, drop_layer tags 200 (_fc1's Dropout, on
 *   act(_fc1.0(x)) [n_tokens, dim], p = fc1_drop_p), 201 (layer 1's to_out Dropout on [1 + H * H, dim], p = attn_drop_p) and
 *   202 (layer 2's, row 0 only: index = column).  p = 0: no mask and no launch for it.  Parity of distribution with torch's
 *   dropout, not of bits. */
typedef struct rrt_transmil_layer_grads {
  float *norm_w, *norm_b;
  rrt_nystrom_grads attn;
} rrt_transmil_layer_grads;

typedef struct rrt_transmil_grads {
  float *fc1_w, *fc1_b;
  float *cls_token;
  rrt_transmil_layer_grads layer[2];
  float *pos_w[3], *pos_b[3];
  float *norm_w, *norm_b;
  float *fc2_w, *fc2_b;
} rrt_transmil_grads;

int rrt_transmil_train_sizes(const rrt_transmil_desc *desc, int64_t n_tokens, size_t *stash_bytes,
                             size_t *backward_workspace_bytes);
int rrt_transmil_forward_train_f32(const rrt_transmil_desc *desc, const rrt_transmil_weights *w, const float *x, float *logits,
                                   int64_t n_tokens, void *stash, size_t stash_bytes, float fc1_drop_p, float attn_drop_p,
                                   uint64_t drop_seed, void *stream);
int rrt_transmil_backward_f32(const rrt_transmil_desc *desc, const rrt_transmil_weights *w, const float *x,
                              const float *d_logits, const void *stash, size_t stash_bytes, const rrt_transmil_grads *grads,
                              float *dx, int64_t n_tokens, void *workspace, size_t workspace_bytes, float fc1_drop_p,
                              float attn_drop_p, uint64_t drop_seed, void *stream);
/* The same step with layer 2's output stage and to_out run for the cls row ALONE (output_row below, a one-row to_out; layer
 * 2's attention stash then holds no o): the other side of the A/B in tools/bench_transmil_train.py.  The same function to
 * rounding.  Not what the step uses: its median was lower in every run measured, but the min-max ranges overlapped in one
 * (DESIGN.md section 8d).  Sizes, stash and workspace are its own; forward and backward must come from the same family. */
int rrt_debug_transmil_train_sizes_row(const rrt_transmil_desc *desc, int64_t n_tokens, size_t *stash_bytes,
                                       size_t *backward_workspace_bytes);
int rrt_debug_transmil_forward_train_row_f32(const rrt_transmil_desc *desc, const rrt_transmil_weights *w, const float *x,
                                             float *logits, int64_t n_tokens, void *stash, size_t stash_bytes, float fc1_drop_p,
                                             float attn_drop_p, uint64_t drop_seed, void *stream);
int rrt_debug_transmil_backward_row_f32(const rrt_transmil_desc *desc, const rrt_transmil_weights *w, const float *x,
                                        const float *d_logits, const void *stash, size_t stash_bytes,
                                        const rrt_transmil_grads *grads, float *dx, int64_t n_tokens, void *workspace,
                                        size_t workspace_bytes, float fc1_drop_p, float attn_drop_p, uint64_t drop_seed,
                                        void *stream);

/* Stage entry points of the step's own kernels.
 *  ppeg_side_backward     : the adjoint of rrt_ppeg_side_f32 WITHOUT the cls row: x, dy [side * side, dim] -> dx (dy plus the
 *                           three transposed depth-wise convs), dw[i] [dim, 1, k, k] for k = 7, 5, 3 and db[i] [dim] (db or
 *                           its entries may be NULL).  w, dw, db: HOST arrays of three DEVICE pointers.  The grid is EXACTLY
 *                           side x side with zero borders, for every side >= 1 (rrt_peg_backward_f32 is the encoder's PPEG,
 *                           which wraps and lifts sides below 7 to 7).  The tap sums are per-tile partials reduced in tile
 *                           order (the kernel of rrt_reduce_partials_f32).  dim % 4 == 0, side <= 1000.
 *  assemble_backward      : the adjoint of the sequence assembly [cls | h | wrap], h = drop(act(hpre)), H = ceil(sqrt(N)):
 *                           d_seq [1 + H * H, dim] -> d_cls [dim] = d_seq[0] and d_emb [n_tokens, dim], row i =
 *                           (d_seq[1 + i] + (i < H * H - N ? d_seq[1 + N + i] : 0)) * mask(tag 200) * act'(hpre[i]): the
 *                           gradient of _fc1's Linear output.  hpre [n_tokens, dim] may be NULL when act is RRT_ACT_NONE.
 *  output_row             : one query row of the output stage, o_row [heads * 64] = softmax(q[row] kl^T) wz +
 *                           sum_t conv_w[h, t] v[row + t - conv_k / 2]; rows outside [0, n_padded) count as zero.
 *  output_row_backward    : d_o_row [heads * 64] -> d_qkv [n_padded, 3 * heads * 64] under output_backward's contract (ALL of it
 *                           written: zero but for row `row` of the q third and the stencil's reach in the v third), d_kl,
 *                           d_wz [heads, 256, 64], d_conv_w [heads, conv_k] (untouched when conv_w is NULL).
 * A row outside [0, n_padded) is RRT_E_UNSUPPORTED with "row" in rrt_strerror. */
int rrt_ppeg_side_backward_workspace_size(int32_t side, int32_t dim, size_t *bytes);
int rrt_ppeg_side_backward_f32(const float *x, const float *dy, const float *const *w, float *dx, float *const *dw,
                               float *const *db, int32_t side, int32_t dim, void *workspace, size_t workspace_bytes,
                               void *stream);
int rrt_transmil_assemble_backward_f32(const float *d_seq, const float *hpre, float *d_emb, float *d_cls, int64_t n_tokens,
                                       int32_t dim, int32_t act, float drop_p, uint64_t drop_seed, void *stream);
int rrt_nystrom_output_row_f32(const float *qkv, const float *kl, const float *wz, const float *conv_w, float *o_row,
                               int64_t row, int64_t n_padded, int32_t heads, int32_t conv_k, void *stream);
int rrt_nystrom_output_row_backward_f32(const float *qkv, const float *kl, const float *wz, const float *conv_w,
                                        const float *d_o_row, float *d_qkv, float *d_kl, float *d_wz, float *d_conv_w,
                                        int64_t row, int64_t n_padded, int32_t heads, int32_t conv_k, void *stream);

/* ---- MHIM-MIL: hard-instance mask selection on the device (Survival/models/MHIM/network.py:480-575, the topk / .tolist() /
 * set arithmetic of select_mask_fn and get_mask as ONE call) and the row movement of the masked student.
 *
 * rrt_mask_select_f32: a [n] the teacher's attention scores, stages [n_stages] (a HOST array; pick is device memory).
 *  Order      for stage s, the n tokens ordered by a: descending if largest, ascending otherwise.  Equal values: the LOWER
 *             index first (-0.0 == +0.0: they tie).  NaN counts as greater than every number, as in torch.topk; NaNs tie
 *             among themselves, by index.
 *  Candidates the first k tokens of that order, 1 <= k <= n.
 *  Pick       the candidate at position j is selected iff pick == NULL or pick[j] != 0; pick is device memory [k].
 *  Result     the selected set is the union over the stages, 1 <= n_stages <= 3.  invert == 0: kept = the complement of the
 *             selected set; invert != 0: kept = the selected set (select_inv).
 *  Outputs    ids [n] (int64): ids[0:count) the kept indices ascending, ids[count:n) the others ascending -- a permutation of
 *             0..n-1, the reference's mask_ids up to the order inside each part.  count [1] (int64, DEVICE memory) the kept
 *             count.  mask [n] (optional, may be NULL) = 1 where dropped, 0 where kept.
 *  The same inputs give the same bits; nothing visits the host; stream-ordered, re-entrant.  workspace:
 *  rrt_mask_select_workspace_size(n, n_stages) bytes (never less for a larger n), else RRT_E_WORKSPACE.  n <= 262144, otherwise
 *  RRT_E_UNSUPPORTED; RRT_E_INVALID on NULL a / stages / ids / count / workspace, n < 1, n_stages outside 1..3, a k outside
 *  1..n.  Every argument is checked before the first launch.
 *
 * rrt_gather_rows_f32:  dst [n_rows, dim] : dst[r, :] = src[ids[r], :], src [n_src, dim].  An id outside [0, n_src) is never
 *  dereferenced; its row is filled with NaN.
 * rrt_scatter_rows_f32: the adjoint.  dst [n_dst, dim] is zero-filled, then dst[ids[r], :] = src[r, :], src [n_rows, dim]; the
 *  ids are distinct, ids outside [0, n_dst) are skipped.
 *  Both: dim % 4 == 0 (else RRT_E_UNSUPPORTED), src and dst 16-byte aligned and not overlapping, sizes >= 1 (RRT_E_INVALID). */
typedef struct rrt_mask_stage {
  int32_t largest;      /* != 0: the k largest scores are the candidates; 0: the k smallest */
  int64_t k;
  const uint8_t *pick;  /* device [k], or NULL = every candidate */
} rrt_mask_stage;
int rrt_mask_select_workspace_size(int64_t n, int32_t n_stages, size_t *bytes);
int rrt_mask_select_f32(const float *a, int64_t n, const rrt_mask_stage *stages, int32_t n_stages, int32_t invert,
                        int64_t *ids, int64_t *count, uint8_t *mask, void *workspace, size_t workspace_bytes, void *stream);
/* rrt_mask_select_vote_f32: the same selection from the per-head attention rows of a multi-head teacher, a [heads, n] row-major
 * (network.py:497-508, msa_fusion='vote': a topk per head, the votes, a topk of the votes with the same k -- as ONE call).
 *  Head order  each head orders the n tokens by its own row under rrt_mask_select_f32's rule (descending if largest, equal
 *              values: the lower index first, -0.0 == +0.0, NaN greatest); a head's candidates are the first k of that order.
 *  Vote        vote[i] = the number of heads that hold token i among their candidates, 0..heads.
 *  Fused order the tokens by vote descending; EQUAL VOTES: THE LOWER INDEX FIRST (torch.topk on the integer votes leaves their
 *              order unspecified, and with two heads nearly every decisive vote is a tie).  The stage's candidates are the first
 *              k of the fused order, 1 <= k <= n; the candidate at position j is selected iff pick == NULL or pick[j] != 0.
 *  Result      union over the stages, invert, ids, count (DEVICE memory) and mask exactly as in rrt_mask_select_f32.  With
 *              heads == 1 and pick == NULL the outputs are those of rrt_mask_select_f32, bit for bit.
 *  The same inputs give the same bits; nothing visits the host; plain launches, integer arithmetic to fixed places, no
 *  atomics; stream-ordered, re-entrant.  workspace: rrt_mask_select_vote_workspace_size(n, heads, n_stages) bytes (never less
 *  for a larger n or for more heads), else RRT_E_WORKSPACE.  1 <= heads <= 16 and n <= 262144, above either RRT_E_UNSUPPORTED;
 *  RRT_E_INVALID on NULL a / stages / ids / count / workspace, n < 1, heads < 1, n_stages outside 1..3, a k outside 1..n.
 *  Every argument is checked before the first launch. */
int rrt_mask_select_vote_workspace_size(int64_t n, int32_t heads, int32_t n_stages, size_t *bytes);
int rrt_mask_select_vote_f32(const float *a, int64_t n, int32_t heads, const rrt_mask_stage *stages, int32_t n_stages,
                             int32_t invert, int64_t *ids, int64_t *count, uint8_t *mask, void *workspace,
                             size_t workspace_bytes, void *stream);
int rrt_gather_rows_f32(const float *src, const int64_t *ids, float *dst, int64_t n_rows, int64_t n_src, int32_t dim,
                        void *stream);
int rrt_scatter_rows_f32(const float *src, const int64_t *ids, float *dst, int64_t n_rows, int64_t n_dst, int32_t dim,
                         void *stream);

/* ---- DTFD-MIL (Survival/models/DTFD/network.py): the double-tier head.  Tier 1 splits the bag into pseudo-bags, pools each
 * with its own softmax attention and picks, per pseudo-bag, the rows with the highest and the lowest class-activation
 * probability; tier 2 is a gated attention pool + classifier over the distilled rows.
 *
 * rrt_gate_scores_f32: a [n_tokens]: a_n = c_w . (hid_a[n] * hid_b[n]) + c_b, hid_* [n_tokens, hidden]; hid_b and c_b may be
 *  NULL.  The arithmetic of rrt_attn_pool_f32's a_raw, bit for bit.  hidden % 4 == 0, n_tokens <= 1e6.
 *
 * rrt_segment_pool_f32: mid [n_tokens, dim], a [n_tokens] scores, perm [n_tokens] int64 (NULL = the identity) the order in
 *  which the rows are dealt to the n_groups groups, cls_w [n_classes, dim] the classifier's weight (no bias: get_cam_1d).
 *  Groups     as np.array_split: q = n_tokens / n_groups, r = n_tokens % n_groups; the first r groups hold q + 1 consecutive
 *             positions of perm, the others q.
 *  Per group  w_i = softmax over the group of a_i;  pooled_g = sum_i w_i mid_i;  p_i = softmax_c(w_i * (mid_i . cls_w_c))[C - 1].
 *  Selection  sel [n_groups, 2] int64 = the ORIGINAL row indices of the group's highest and lowest p, in that order.  Among
 *             equal p the LOWER POSITION IN GROUP ORDER wins, at both ends; -0 == +0; a NaN p is never selected; a group
 *             whose every p is NaN selects its first member at both ends; a group of one selects that member twice.
 *  Outputs    pooled [n_groups, dim], sel; optional (NULL: not wanted) attn [n_tokens] = w and p [n_tokens], both written at
 *             the original row index.  A perm entry outside [0, n_tokens) is never dereferenced: its row counts as NaN.
 *  fp32 with accurate expf whatever mode the caller's GEMMs run in; every sum has a fixed order (same inputs, same bits); no
 *  atomics; nothing visits the host; stream-ordered, re-entrant.
 * rrt_segment_pool_backward_f32: the pooling's adjoint.  With c_g = pooled_g . d_pooled_g:  d_mid_i = w_i d_pooled_g and
 *  d_a_i = w_i (mid_i . d_pooled_g - c_g), written at the original row indices (every row belongs to one group).  The
 *  selection is an integer output without an adjoint: what reaches mid through the selected rows is the caller's
 *  (rrt_scatter_rows_f32, or torch's index_select).  `workspace` is the one the forward call with the same mid / a / perm /
 *  sizes left behind: the groups' (m_g, l_g) = (max score, softmax denominator) are its first 2 * n_groups floats.
 * Limits (RRT_E_UNSUPPORTED from the size query and from the calls alike, before anything is launched): dim % 32 == 0,
 *  dim <= 2048, 1 <= n_classes <= 8, 1 <= n_groups <= 64, n_groups <= n_tokens <= 1e6 (the reference tolerates
 *  n_tokens < group -- empty chunks add no rows --, this library refuses it and says so).  RRT_E_INVALID on NULL / non-positive
 *  arguments or pointers that are not 16-byte aligned, RRT_E_WORKSPACE below rrt_segment_pool_workspace_size bytes. */
int rrt_segment_pool_workspace_size(int64_t n_tokens, int32_t dim, int32_t n_classes, int32_t n_groups, size_t *bytes);
int rrt_gate_scores_f32(const float *hid_a, const float *hid_b, const float *c_w, const float *c_b, float *a,
                        int64_t n_tokens, int32_t hidden, void *stream);
int rrt_segment_pool_f32(const float *mid, const float *a, const int64_t *perm, const float *cls_w, float *pooled,
                         int64_t *sel, float *attn, float *p, int64_t n_tokens, int32_t dim, int32_t n_classes,
                         int32_t n_groups, void *workspace, size_t workspace_bytes, void *stream);
int rrt_segment_pool_backward_f32(const float *mid, const float *a, const int64_t *perm, const float *pooled,
                                  const float *d_pooled, float *d_mid, float *d_a, int64_t n_tokens, int32_t dim,
                                  int32_t n_groups, void *workspace, size_t workspace_bytes, void *stream);

/* DTFD.test_forward as one call (eval, one bag, one stream): x [n_tokens, input_dim] -> fc1 (no bias) + act -> RRTEncoder
 * over the whole bag (has_rrt) -> the two gate Linears tanh / sigmoid (enc.compute's arithmetic, as the
 * RRT_BAGPOOL_ATTN_GATED tail) -> rrt_gate_scores_f32 -> rrt_segment_pool_f32 over perm -> the distilled rows
 * (rrt_gather_rows_f32 by the ids the selection wrote) -> tier 2 (the path behind rrt_pool_predict_f32: gated, tanh) ->
 * logits [n_classes].  sigmoid / cumprod of the logits stay with the caller.  Nothing visits the host.
 *   RRT_DTFD_MAXMINS  tier 2 sees [mid[imax_g], mid[imin_g]] for g = 0 .. group - 1   (2 * group rows)
 *   RRT_DTFD_MAXS     mid[imax_g]                                                      (group rows)
 *   RRT_DTFD_AFS      pooled_g                                                         (group rows)
 * Optional outputs (NULL: not wanted): sel [group, 2] int64, p [n_tokens] the CAM probability of every row (the heat map).
 * Limits: those of the heads' front (rrt_bagmil_forward_f32), of rrt_segment_pool_f32 and of rrt_pool_predict_f32. */
enum { RRT_DTFD_MAXMINS = 0, RRT_DTFD_MAXS = 1, RRT_DTFD_AFS = 2 };
typedef struct rrt_dtfd_desc {
  rrt_encoder_desc enc;    /* has_rrt = 0: only dim (= 512 in the reference) and compute are read */
  int32_t input_dim;       /* patch feature width (multiple of 32) */
  int32_t emb_act;         /* RRT_ACT_RELU / RRT_ACT_GELU (RRT_ACT_NONE is accepted) */
  int32_t has_rrt;
  int32_t n_classes;       /* 1..8 */
  int32_t hidden;          /* D of both Attention blocks: 128 in the reference (multiple of 4) */
  int32_t group;           /* pseudo-bags, 1..64 */
  int32_t distill;         /* RRT_DTFD_* */
} rrt_dtfd_desc;
typedef struct rrt_dtfd_weights {
  rrt_encoder_weights enc;
  const float *emb_w;                  /* dimReduction.fc1.weight              [dim, input_dim] (no bias) */
  const float *att_v_w, *att_v_b;      /* attention.attention_V.0              [hidden, dim], [hidden] */
  const float *att_u_w, *att_u_b;      /* attention.attention_U.0              [hidden, dim], [hidden] */
  const float *att_w_w, *att_w_b;      /* attention.attention_weights          [1, hidden], [1] */
  const float *cls_w;                  /* classifier.fc.weight                 [n_classes, dim] (its bias plays no part in eval) */
  const float *u_v_w, *u_v_b;          /* UClassifier.attention.attention_V.0  [hidden, dim], [hidden] */
  const float *u_u_w, *u_u_b;          /* UClassifier.attention.attention_U.0 */
  const float *u_w_w, *u_w_b;          /* UClassifier.attention.attention_weights [1, hidden], [1] */
  const float *u_fc_w, *u_fc_b;        /* UClassifier.classifier.fc            [n_classes, dim], [n_classes] */
} rrt_dtfd_weights;
int rrt_dtfd_workspace_size(const rrt_dtfd_desc *desc, int64_t n_tokens, size_t *bytes);
int rrt_dtfd_forward_f32(const rrt_dtfd_desc *desc, const rrt_dtfd_weights *w, const float *x, const int64_t *perm,
                         float *logits, int64_t *sel, float *p, int64_t n_tokens, void *workspace, size_t workspace_bytes,
                         void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RRT_HIP_H */
