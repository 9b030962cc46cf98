// api.hip -- the C ABI of librrt_hip.so (include/rrt_hip.h) around the encoder: error strings, geometry, workspace carving, the
// kernel plan and launch sequence of one RRTEncoder forward (modules/rrt.py:165-202), the stage entries, the heads, the
// batch-of-bags executor and the encoder's training.  Nystrom attention and TransMIL live in api_nystrom.hip.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "api_internal.h"

using namespace rrt_api;

namespace {

thread_local char g_detail[256] = "";

int64_t ceil_sqrt(int64_t n) {
  int64_t r = (int64_t)floor(sqrt((double)n));
  while (r * r > n) --r;
  while ((r + 1) * (r + 1) <= n) ++r;
  return r * r == n ? r : r + 1;
}

struct Workspace {
  float *uo, *qkv, *xa, *xb, *mean_rstd, *logits, *wdisp, *rep, *rep_qkv, *rep_o, *rep2, *v8, *hid;
  float *ffn_ln, *ffn_hid, *xp;
  float* pe_out;     // value-EPEG ablation: the conv's output [Np, D]
  float* smap;       // 2-D 'attn' EPEG on regions whose [P, P] score map does not fit the LDS: the maps [R * heads][P][P]
  uint16_t* w16;     // reduced-precision modes: 16-bit copies of the R-MSA layers' qkv / proj weights (4 D^2 per layer)
  uint16_t* wcr16;   // ... and of CR-MSA's inner qkv / proj weights (4 D^2), bf16 / fp16 modes
  uint16_t *rep16, *repo16;   // 16-bit representatives [k * 64, D] and their attention output (the fused 16-bit inner MSA)
  float* cr_part;    // crmsa_region4_kernel: partial records of the region quarters
  int* cr_cnt;       // ... and the 64 arrival counters (zeroed by an R-MSA GEMM of the same forward)
  int* proj_cnt;     // rmsa_fused_kernel<.., PROJ>: one arrival counter per region (zeroed by the layer's LayerNorm + partition)
  float* cr_pstat;   // row records of the last R-MSA layer's projection slabs [N][D / 64][2 + k] (crmsa_combine_parts_kernel)
  size_t bytes;
};

// One carve function used for both the size query (base = null) and the real carve.
Workspace carve(const rrt_encoder_desc& d, int64_t N, const rrt_grid& g, const rrt_grid& g8, char* base) {
  Workspace w{};
  Arena a{base};
  const size_t D = d.dim;
  const size_t Np = (size_t)g.H * g.H, Np8 = (size_t)g8.H * g8.H;
  const size_t R8 = (size_t)g8.regions_side * g8.regions_side;
  // the weight images first, so that their place does not depend on n_tokens (desc.weights16_valid)
  if (d.n_rmsa_layers > 0) w.w16 = (uint16_t*)a.take((size_t)d.n_rmsa_layers * 4 * D * D);     // (F32X3: (hi, lo) pairs = 4 bytes per weight)
  if (d.cr_msa) w.wcr16 = (uint16_t*)a.take(2 * D * D);                                         // 4 D^2 16-bit weights
  if (d.n_rmsa_layers > 0) {
    // w16: its place does not depend on n_tokens (desc.weights16_valid); carved in every mode (4 D^2 floats
    // = 4 MiB per layer at D = 512): the size must not depend on desc.compute, which callers flip between calls on one
    // workspace
    w.uo = a.take(Np * D);
    w.qkv = a.take(Np * 3 * D);
    w.xa = a.take((size_t)N * D);
    if (d.n_rmsa_layers > 1 || d.ffn) w.xb = a.take((size_t)N * D);
    w.proj_cnt = (int*)a.take((size_t)g.regions_side * g.regions_side);
    if (d.epeg && d.epeg_type != RRT_EPEG_ATTN) w.pe_out = a.take(Np * D);
    if (d.epeg && d.epeg_2d && d.epeg_type == RRT_EPEG_ATTN) {
      const size_t sm = attn_scoremap_scratch_floats(g.regions_side * g.regions_side, g.s * g.s, d.n_heads, d.epeg_k, 1);
      if (sm) w.smap = a.take(sm);
    }
  }
  if (d.ffn) {
    if (!w.xa) w.xa = a.take((size_t)N * D);
    if (!w.xb) w.xb = a.take((size_t)N * D);
    w.ffn_ln = a.take((size_t)N * D);
    w.ffn_hid = a.take((size_t)N * d.ffn_hidden);
  }
  if (d.cr_msa) {
    const size_t k = d.crmsa_k;
    w.mean_rstd = a.take((size_t)N * 2);
    w.logits = a.take(Np8 * k);
    w.wdisp = a.take(Np8 * k);
    w.rep = a.take(k * R8 * D);
    w.rep_qkv = a.take(k * R8 * 3 * D);
    w.rep_o = a.take(k * R8 * D);
    w.rep2 = a.take(k * R8 * D);
    w.rep16 = (uint16_t*)a.take(k * R8 * D / 2);
    w.repo16 = (uint16_t*)a.take(k * R8 * D / 2);
    if (d.n_rmsa_layers > 0) {
      w.cr_part = a.take(crmsa_region4_scratch_floats(to_dev(g8), d.crmsa_k));
      w.cr_cnt = (int*)a.take(64);
      if (D % 64 == 0) w.cr_pstat = a.take(crmsa_parts_floats(N, (int)D, d.crmsa_k));
    }
    if (d.crmsa_mlp) {
      w.v8 = a.take(Np8 * D);
      w.hid = a.take(Np8 * (D / 4));
    }
  }
  if (d.pos) w.xp = a.take((size_t)N * D);
  w.bytes = a.bytes() ? a.bytes() : 256;
  return w;
}

}  // namespace

// what api_nystrom.hip calls too (api_internal.h)
namespace rrt_api {

int unsupported(const char* why) {
  snprintf(g_detail, sizeof(g_detail), "%s", why);
  return RRT_E_UNSUPPORTED;
}

// the dropout configuration of one training call (DropCfg: api_internal.h)
int make_drop(float p, DropCfg* d) {
  if (!(p >= 0.f) || p >= 1.f) return RRT_E_INVALID;
  d->thresh = p > 0.f ? (unsigned)((double)p * 4294967296.0) : 0u;
  if (p > 0.f && d->thresh == 0) d->thresh = 1;
  d->scale = 1.0f / (1.0f - p);
  return RRT_OK;
}

}  // namespace rrt_api

namespace {

int check_desc(const rrt_encoder_desc* d, int64_t N) {
  if (!d || N <= 0) return RRT_E_INVALID;
  if (d->dim <= 0 || d->dim % 32 != 0) return unsupported("dim must be a positive multiple of 32");
  if (d->dim > 2048) return unsupported("dim > 2048");
  if (d->n_rmsa_layers < 0 || d->n_rmsa_layers > RRT_MAX_RMSA_LAYERS) return unsupported("n_layers-1 out of range");
  if (d->n_rmsa_layers > 0) {
    if (d->n_heads <= 0 || d->dim % d->n_heads != 0) return unsupported("n_heads must divide dim");
    if (d->epeg && (d->epeg_k <= 0 || d->epeg_k % 2 == 0)) return unsupported("epeg_k must be odd");
    if (d->epeg_type < RRT_EPEG_ATTN || d->epeg_type > RRT_EPEG_VALUE_AF) return unsupported("epeg_type must be attn / value_bf / value_af");
    if (d->epeg && (d->epeg_2d || d->epeg_type != RRT_EPEG_ATTN) && d->epeg_k > 63) return unsupported("epeg ablations: epeg_k <= 63");
    if (d->region_size <= 0 && d->region_num <= 0) return unsupported("region_num must be positive");
  }
  if (d->cr_msa) {
    if (d->crmsa_k <= 0 || d->crmsa_k > RRT_MAX_CRMSA_K) return unsupported("crmsa_k must be in [1,8]");
    if (d->crmsa_heads <= 0 || d->dim % d->crmsa_heads != 0) return unsupported("crmsa_heads must divide dim");
  }
  if (d->ffn) {
    if (d->ffn_hidden <= 0 || d->ffn_hidden % 32 != 0)
      return unsupported("ffn: hidden width int(dim * mlp_ratio) must be a positive multiple of 32");
    if (d->ffn_act != RRT_ACT_GELU && d->ffn_act != RRT_ACT_RELU) return unsupported("ffn_act must be gelu or relu");
  }
  if (d->pos) {
    if (d->pos != RRT_POS_PEG && d->pos != RRT_POS_PPEG) return unsupported("pos must be none / peg / ppeg");
    if (d->peg_k <= 0 || d->peg_k % 2 == 0 || d->peg_k > 11) return unsupported("peg_k must be odd and <= 11");
    if (d->pos_pos != -1 && d->pos_pos != 0) return unsupported("pos_pos must be -1 or 0");
  }
  if (N > (int64_t)4000000) return unsupported("bag larger than 4e6 tokens");
  if (d->compute < 0 || d->compute > RRT_COMPUTE_F32X3) return unsupported("compute must be RRT_COMPUTE_F32/BF16/F16/F32X3");
  return RRT_OK;
}

// The two grids every encoder entry point needs -- the R-MSA layers' (g; zero when there is no such layer) and CR-MSA's, which
// never receives region_num / region_size / min_region_* (modules/rrt.py:148): 8 x 8 -- and check_desc in front of them.
int region_grids(const rrt_encoder_desc* d, int64_t N, rrt_grid* g, rrt_grid* g8) {
  *g = rrt_grid{};
  if (d->n_rmsa_layers > 0) {
    int rc = rrt_region_grid(N, d->region_num, d->region_size, d->min_region_num, d->min_region_ratio, g);
    if (rc) return rc;
  }
  return rrt_region_grid(N, 8, 0, 0, 0.f, g8);
}
// (an entry point with conditions of its own between the two steps calls them one by one: the order decides which error a
// call with several faults reports)
int resolve_grids(const rrt_encoder_desc* d, int64_t N, rrt_grid* g, rrt_grid* g8) {
  int rc = check_desc(d, N);
  return rc ? rc : region_grids(d, N, g, g8);
}

// one region that holds the whole bag in token order: slot == token, for GEMMs whose residual is not partitioned (the FFN)
GridDev identity_grid(int64_t N) {
  GridDev g{};
  const int Hs = (int)ceil_sqrt(N);
  g.L = (int)N;
  g.H = g.s = Hs;
  g.rs = 1;
  g.P = g.Np = Hs * Hs;
  g.inv_H = g.inv_s = 1.0f / (float)Hs;
  g.inv_rs = 1.0f;
  g.inv_P = 1.0f / (float)g.P;
  g.Rt = 1;
  return g;
}

// epilogue of a qkv projection: bias, then the q columns scaled by head_dim ** -0.5 (modules/rmsa.py:65,103)
LinearEpilogue qkv_epilogue(const float* bias, int dim, int heads, int prec) {
  LinearEpilogue ep{};
  ep.prec = prec;
  ep.bias = bias;
  ep.q_cols = dim;
  ep.q_scale = 1.0f / sqrtf((float)(dim / heads));
  return ep;
}

// epilogue of an out-projection: bias, un-partition by g, residual (rmsa.py:131,41-54; rrt.py:125)
LinearEpilogue proj_epilogue(const float* bias, const float* resid, const GridDev& g, int prec) {
  LinearEpilogue ep{};
  ep.prec = prec;
  ep.bias = bias;
  ep.resid = resid;
  ep.g = g;
  return ep;
}

hipError_t inner_attention(const float* u, int n_regions, int P, const rrt_attn_weights& w, int dim,
                           int heads, int epeg_k, float* qkv, float* o, int prec, bool solo, hipStream_t st) {
  const int M = n_regions * P;
  LinearEpilogue ep = qkv_epilogue(w.qkv_b, dim, heads, prec);
  ep.solo = solo;
  hipError_t e = launch_linear(u, w.qkv_w, qkv, M, 3 * dim, dim, ep, st);
  if (e != hipSuccess) return e;
  return launch_region_attention(qkv, epeg_k > 0 ? w.pe_w : nullptr, o, n_regions, P, dim, heads,
                                 epeg_k, st);
}

// ---- the kernel plan of one forward: which launch sequence its R-MSA layers and its CR-MSA front take.  A pure function of
// the descriptor, the two grids and "the call stops before CR-MSA" (no workspace pointer, no state between calls):
// encoder_forward launches from it, rrt_encoder_plan reports it.  Where a kernel needs a workspace buffer that carve() only
// hands out under a condition, that condition is restated here next to carve's name.
enum class LayerKind {
  Pair16Merged,   // 16-bit pair kernel with the out-projection as a phase of its launch (tuning builds only)
  Fused16,        // 16-bit fused kernel, then the out-projection on 16-bit operands
  FusedX3,        // RRT_COMPUTE_F32X3: fused kernel and out-projection on split (hi, lo) bf16 images
  EpegVariant,    // EPEG ablations (epeg_2d, epeg_type = value_*): unfused, with their own kernels (epeg_variants.hip)
  FusedProj,      // exact fp32: fused kernel with the out-projection as a later phase of the same launch
  Fused,          // fused kernel, then the out-projection GEMM
  Unfused,        // qkv GEMM, region attention, out-projection GEMM
};
enum class FrontKind { None, Mlp, Parts, RegionInFlight, Region4, Region, Stream4, TwoKernel };
enum class CastKind { None, Images16, Split };
struct EncoderPlan {
  LayerKind layer;   // of every R-MSA layer (they share shape and mode); not looked at when there is none
  bool parts;        // the last R-MSA layer also leaves the CR-MSA row records (FusedProj only)
  bool gated;        // the layer's core launch takes the phase gate when the call has one
  bool attn_hd;      // Unfused: the attention is region_attn_hd's (launch_region_attention decides that; reported only)
  CastKind casts;    // the R-MSA layers' weight images this call writes
  bool inner16;      // CR-MSA's inner MSA on the 16-bit kernels (its weight images ride with the cast launch)
  FrontKind front;   // CR-MSA's first pass: logits + combine
  int rows_w;        // > 0: LayerNorm + partition (K1) and dispatch + final LayerNorm (K7) take their row-looping forms on a
                     // grid of rows_w waves per SIMD (ln_partition.hip, crmsa.hip); 0: a wave per row
  bool rows_ln1;     // ... K1 as well (the exact fp32 layers; the 16-bit modes have their own LayerNorm + partition)
};

// Waves per SIMD of the row-looping K1 / K7 (ROWS_W_MAX = 3).  Default bench (N = 9000, fp32, four bags in flight), one box,
// five rounds alternating, medians in slides/s: a wave per row 5350 (parent commit) / 5350 (tuning build, RRT_ROWS_W=0),
// w = 1 5431, w = 2 5410, w = 3 5389; the parent's own spread was 13 (profiles/rows_in_flight_ab.txt).
constexpr int ROWS_W_DEFAULT = 1;

// smallest CR-MSA region (tokens) that takes crmsa_stream4_kernel instead of crmsa_region4_kernel (A/B builds:
// -DRRT_STREAM4_MIN_P=16)
#ifndef RRT_STREAM4_MIN_P
#define RRT_STREAM4_MIN_P 145
#endif

EncoderPlan plan_encoder(const rrt_encoder_desc& d, const rrt_grid& g, const rrt_grid& g8, bool stops_before_crmsa) {
  EncoderPlan p{};
  p.layer = LayerKind::Unfused;
  const int D = d.dim;
  // RRT_COMPUTE_F32X3 concerns the R-MSA layers' two big projections; everything else of the call is exact fp32
  const bool want_x3 = d.compute == RRT_COMPUTE_F32X3;
  const int compute = want_x3 ? RRT_COMPUTE_F32 : d.compute;
  // Reduced-precision modes: every tensor that is only a matrix-core operand (LayerNorm output u, the weights, the attention
  // output O) lives in HBM in 16 bits; 64-element K tiles
  const bool lowp = compute != RRT_COMPUTE_F32 && D % 64 == 0;
  const GridDev gd8 = to_dev(g8);
  // CR-MSA's inner MSA over the 64 k representatives on the same 16-bit kernels (one fused launch + one GEMM instead
  // of GEMM + attention + GEMM on fp32 data): head dim 64 only (crmsa_heads = dim / 64)
  p.inner16 = d.cr_msa && lowp && rmsa_fused16_supported(64, D, d.crmsa_heads, 0);
  // K1 / K7 with bags in flight (exact fp32, solo = 0): the row-looping forms -- a launch that is resident at once beside
  // another bag's fused R-MSA blocks and sends the dispatcher no further waves.  dim <= 512 and crmsa_k <= 3 only: the other
  // instantiations need more than the 72 VGPRs two such waves have beside two fused waves of a SIMD (90 / 111 at k <= 5 / 8).
  // One bag in flight keeps a wave per row (latency-optimal there).  The 16-bit modes keep it too (their K1 is another
  // kernel; K7 alone in the row-looping form was measured with RRT_ROWS_LOWP: the bf16 lines of profiles/rows_in_flight_ab.txt).
  // Tuning build: RRT_ROWS_W = 0 (a wave per row everywhere) .. 3; RRT_ROWS_LOWP: K7 of the 16-bit modes as well.
  {
    static const char* rows_env = rrt_tune_env("RRT_ROWS_W");
    static const bool rows_lowp = rrt_tune_env("RRT_ROWS_LOWP") != nullptr;
    int w = ROWS_W_DEFAULT;
    if (rows_env != nullptr && atoi(rows_env) >= 0 && atoi(rows_env) <= ROWS_W_MAX) w = atoi(rows_env);
    const bool exact = d.compute == RRT_COMPUTE_F32;
    const bool fits = D <= 512 && (!d.cr_msa || d.crmsa_k <= 3);
    if (!d.solo && fits && (exact || (rows_lowp && lowp))) {
      p.rows_w = w;
      p.rows_ln1 = exact && w > 0;
    }
  }
  if (d.n_rmsa_layers > 0) {
    const GridDev gd = to_dev(g);
    const int R = gd.rs * gd.rs, heads = d.n_heads, ek = d.epeg ? d.epeg_k : 0;
    const bool rows_ok = rmsa_fused_supported_rows(gd.Np, D);
    static const bool want_merged16 = rrt_tune_env("RRT_PAIR16_PROJ") != nullptr;
    if (d.epeg && (d.epeg_2d || d.epeg_type != RRT_EPEG_ATTN)) {
      p.layer = LayerKind::EpegVariant;
    } else if (lowp && rmsa_fused16_supported(gd.P, D, heads, ek) && rows_ok) {
      // round 6: bags of at least two rounds of (pair, head) items (N = 30000 at region_num = 16: four) CAN take the
      // out-projection as a phase of the pair launch's blocks (rmsa_pair16.hip, PROJ; bit-identical, tested) -- built on the
      // round-5 review's request and MEASURED SLOWER than the two launches: 109-116 us against 64.5 + 35.6 at N = 30000
      // (profiles/r06_trace_pair16_proj.txt: a slab costs a block 25 K cycles -- 13 K of DMA-issue-bound K loop, the same
      // bound the separate projection runs at with two blocks per CU hiding each other's prologue and epilogue -- plus 4 K
      // waiting for the write-through O stores; the block owns its CU, so nothing overlaps the slab).  Off unless a tuning
      // build asks for it (RRT_PAIR16_PROJ=1).  (carve: its arrival counters, proj_cnt, exist whenever n_rmsa_layers > 0)
      p.layer = want_merged16 && rmsa_pair16_proj_supported(R, gd.P, D, heads, ek) ? LayerKind::Pair16Merged : LayerKind::Fused16;
    } else if (want_x3 && D % 256 == 0 && rmsa_fused_x3_supported(gd.P, D, heads, ek) && rows_ok) {
      // the qkv and proj GEMMs emulated in fp32 on the bf16 matrix cores (operands as (hi, lo) bf16 pairs, three MFMAs per
      // product; rmsa_fused_x3.hip, cast16.hip); attention and everything else as F32.
      // dim % 256 == 0 only: at other widths the LayerNorm-type kernels keep their lane-predicated column guards, and those
      // mis-summed now and then with split-kernel waves co-resident (root cause not established) -- such
      // widths get the exact fp32 kernels instead (more accurate than what was asked for)
      p.layer = LayerKind::FusedX3;
    } else if (compute == RRT_COMPUTE_F32 && rows_ok && rmsa_fused_proj_supported(R, gd.P, D, heads, ek, compute)) {
      // the exact fp32 path of bags that fill the chip twice over: fused R-MSA kernel with the out-projection + un-partition
      // + residual as a later phase of the same launch's blocks (rmsa_fused.hip, PROJ): one launch per R-MSA layer
      // (carve: proj_cnt, as above)
      p.layer = LayerKind::FusedProj;
      // CR-MSA's first pass as a by-product of the last R-MSA layer's projection slabs: that layer's output must BE CR-MSA's
      // input (no FFN behind the attention, not the batch entry point's per-bag stop), phi a plain parameter, 64-column slabs
      // (carve: the records, cr_pstat, exist when cr_msa, n_rmsa_layers > 0 and dim % 64 == 0) -- and the forward has the GPU
      // to itself (rrt_encoder_desc.solo): the statistics cost the merged launch ~3 us of matrix-pipe time and save ~6 us of
      // the latency-bound CR-MSA front -- one bag in flight 0.2238 -> 0.2218 ms, but with four bags in flight the tail hides
      // behind other bags' tails anyway and the matrix pipe is the scarce thing: 5.26 k against 5.31 k slides/s (round 5,
      // same box); likewise k > 4 representatives (twice the record) stay with the region kernels
      p.parts = d.solo != 0 && d.cr_msa && !d.crmsa_mlp && !d.ffn && d.crmsa_k <= 4 && !stops_before_crmsa && D % 64 == 0 &&
                crmsa_combine_parts_supported(D, d.crmsa_k, gd8);
    } else if (rmsa_fused_supported(gd.P, D, heads, ek) && rows_ok) {
      // qkv projection + EPEG + attention in one kernel per (region, head): qkv never reaches HBM
      p.layer = LayerKind::Fused;
    } else {
      p.attn_hd = region_attention_hd_supported(gd.P, D, heads, ek);
    }
    // the gate only pays for launches that fill the matrix pipes of the whole chip on their own: the fused
    // kernels on regions of >= 113 tokens (measured on the configs[4] mix: gating small or unfused bags costs 5 %)
    p.gated = gd.P > 112 && p.layer != LayerKind::EpegVariant && p.layer != LayerKind::Unfused;
    // The images are written whenever a reduced / emulated mode is asked for -- whether or not THIS bag's regions take the
    // 16-bit kernels: the workspace (and the caller's validity key) outlives the bag, and the next, smaller bag on it may
    // take them (a 20 k-token bag followed by a 9 k-token one).
    if (p.layer != LayerKind::EpegVariant) p.casts = lowp ? CastKind::Images16 : want_x3 ? CastKind::Split : CastKind::None;
  }
  if (!d.cr_msa || stops_before_crmsa) return p;
  const int k = d.crmsa_k;
  // carve: crmsa_region4 / crmsa_stream4's partial records and arrival counters (cr_part, cr_cnt) exist when there is an R-MSA
  // layer -- whose out-projection also zeroes the counters
  const bool has_counters = d.n_rmsa_layers > 0;
  static const bool no_region_inflight = rrt_tune_env("RRT_NO_REGION_INFLIGHT") != nullptr;
  static const bool region_lowp = rrt_tune_env("RRT_REGION_INFLIGHT_LOWP") != nullptr;      // (A/B: also in the 16-bit modes)
  if (d.crmsa_mlp) {
    p.front = FrontKind::Mlp;
  } else if (p.parts) {
    p.front = FrontKind::Parts;
  } else if (!no_region_inflight && !d.solo && p.layer != LayerKind::FusedX3 && (compute == RRT_COMPUTE_F32 || region_lowp) &&
             crmsa_region_supported(D, k, gd8)) {
    // round 6: exact fp32 with SEVERAL bags in flight -- logits + combine as ONE sixteen-wave block per region
    // (crmsa_region_kernel, its k = 1 .. 3 forms with gamma . phi in registers): 64 blocks, so three quarters of the chip stay
    // with the other bags' fused R-MSA launches, which is what the line is made of (the fused launches' union is 187 of the
    // 189 us a bag takes).  Same box, four bags in flight: 5.30-5.31 k -> 5.36-5.38 k slides/s with the round-1 kernel
    // (profiles/r06_region1_in_flight_ab.txt); one bag in flight it loses (20 us on a quarter of the chip): the hint decides.
    // The 16-bit modes keep crmsa_region4 (their chip-wide kernels are short: a 64-block front becomes the critical path).
    p.front = FrontKind::RegionInFlight;
  } else if (has_counters && crmsa_region4_supported(D, k, gd8) && gd8.P < RRT_STREAM4_MIN_P) {
    // logits + combine in one pass over x1: four blocks per region, the last to arrive merges (crmsa_region4_kernel).
    // Regions of more than 144 tokens (8 / 16 blocks per region: the kernel covers them, tests) stay with the two chip-wide
    // kernels: measured on MI355X (tools/bench_crmsa.py) the merge of 8-16 partial records per region costs more than the
    // second pass over x1 -- N = 15000: 36 vs 24 us, N = 30000: 46-74 vs 39 us.
    p.front = FrontKind::Region4;
  } else if (crmsa_region_enabled() && crmsa_region_supported(D, k, gd8)) {
    p.front = FrontKind::Region;
  } else if (has_counters && gd8.P >= RRT_STREAM4_MIN_P && crmsa_stream4_supported(D, k, gd8)) {
    // round 6: regions of more than 144 tokens in ONE pass over x1 as well -- four blocks per region that stream their rows
    // with an online softmax per wave, crmsa_region4's records and merge (crmsa_stream4_kernel)
    p.front = FrontKind::Stream4;
  } else {
    p.front = FrontKind::TwoKernel;
  }
  return p;
}

}  // namespace

GridDev to_dev(const rrt_grid& g) {
  GridDev d;
  d.L = (int)g.L;
  d.H = g.H;
  d.s = g.s;
  d.rs = g.regions_side;
  d.P = g.s * g.s;
  d.Np = g.H * g.H;
  d.inv_H = 1.0f / (float)d.H;
  d.inv_s = 1.0f / (float)d.s;
  d.inv_rs = 1.0f / (float)d.rs;
  d.inv_P = 1.0f / (float)d.P;
  d.Rt = d.rs * d.rs;
  return d;
}

extern "C" {

int rrt_abi_version(void) { return RRT_ABI_VERSION; }

const char* rrt_strerror(int code) {
  switch (code) {
    case RRT_OK: return "ok";
    case RRT_E_INVALID: return "invalid argument (null pointer or non-positive size)";
    case RRT_E_UNSUPPORTED: return g_detail[0] ? g_detail : "unsupported configuration";
    case RRT_E_WORKSPACE: return "workspace too small (see rrt_encoder_workspace_size)";
    case RRT_E_HANDOVER: return "an earlier merged R-MSA launch gave up its in-launch hand-over wait; outputs in flight are invalid "
                                "(synchronise, then rrt_device_error(1) to clear)";
    default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown error";
  }
}

int rrt_region_grid(int64_t L, int32_t region_num, int32_t region_size, int32_t min_region_num,
                    float min_region_ratio, rrt_grid* out) {
  if (!out || L <= 0) return RRT_E_INVALID;
  if (region_size <= 0 && region_num <= 0) return RRT_E_INVALID;
  int64_t H = ceil_sqrt(L), s;
  if (region_size > 0) {
    H += ((-H) % region_size + region_size) % region_size;
    s = region_size;
  } else {
    H += ((-H) % region_num + region_num) % region_num;
    s = H / region_num;
  }
  int64_t add = H * H - L;
  // "if padding much, give up region attention" (ablation escape hatch, rmsa.py:191-196);
  // evaluated in double like the reference's Python floats
  if ((double)add > (double)L / ((double)min_region_ratio + 1e-8) || L < min_region_num) {
    H = ceil_sqrt(L);
    H += H % 2;
    add = H * H - L;
    s = H;
  }
  if (H > 46340) return RRT_E_INVALID;
  out->L = L;
  out->H = (int32_t)H;
  out->s = (int32_t)s;
  out->regions_side = (int32_t)(H / s);
  out->add = add;
  return RRT_OK;
}

int rrt_encoder_workspace_size(const rrt_encoder_desc* desc, int64_t n_tokens, size_t* bytes) {
  if (!bytes) return RRT_E_INVALID;
  rrt_grid g{}, g8{};
  int rc = resolve_grids(desc, n_tokens, &g, &g8);
  if (rc) return rc;
  *bytes = carve(*desc, n_tokens, g, g8, nullptr).bytes;
  return RRT_OK;
}

// The forward's own plan (plan_encoder) for the R-MSA layers, as RRT_PLAN_* bits; measurement only.
int rrt_encoder_plan(const rrt_encoder_desc* desc, int64_t n_tokens, int32_t* flags) {
  if (!flags) return RRT_E_INVALID;
  *flags = 0;
  rrt_grid g{}, g8{};
  int rc = resolve_grids(desc, n_tokens, &g, &g8);
  if (rc) return rc;
  if (desc->n_rmsa_layers <= 0) return RRT_OK;
  const EncoderPlan plan = plan_encoder(*desc, g, g8, false);
  switch (plan.layer) {
    case LayerKind::Pair16Merged:
    case LayerKind::Fused16: *flags = RRT_PLAN_FUSED16; break;
    case LayerKind::FusedX3: *flags = RRT_PLAN_FUSED_X3; break;
    case LayerKind::FusedProj: *flags = RRT_PLAN_FUSED | RRT_PLAN_FUSED_PROJ | (plan.parts ? RRT_PLAN_CRMSA_PARTS : 0); break;
    case LayerKind::Fused: *flags = RRT_PLAN_FUSED; break;
    case LayerKind::Unfused: *flags = plan.attn_hd ? RRT_PLAN_ATTN_HD : 0; break;      // qkv linear + region_attn_hd
    case LayerKind::EpegVariant: break;
  }
  return RRT_OK;
}

// ... and for the two streaming stages around them (its own entry point: the flag word above is compared for equality by its
// users, bench.py among them)
int rrt_encoder_plan_rows(const rrt_encoder_desc* desc, int64_t n_tokens, int32_t* w) {
  if (!w) return RRT_E_INVALID;
  *w = 0;
  rrt_grid g{}, g8{};
  int rc = resolve_grids(desc, n_tokens, &g, &g8);
  if (rc) return rc;
  *w = plan_encoder(*desc, g, g8, false).rows_w;
  return RRT_OK;
}

// Serialises the MFMA-bound R-MSA core (fused kernel, or qkv linear + attention) of forwards that run
// concurrently on different streams: two of them co-running just time-slice the matrix pipes (each takes
// twice as long), while one of them next to another bag's memory- and latency-bound kernels overlaps well.
struct rrt_phase_gate {
  hipEvent_t done;     // completion of the most recent gated phase (any stream)
  bool armed;
};

// TransLayer's optional FFN (rrt.py:127-129): xo = xi + fc2(act(fc1(LN2(xi)))).  LN2 -> GEMM with the activation in its
// epilogue -> GEMM with the residual in its epilogue (identity slot -> token map).
static int ffn_apply(const rrt_encoder_desc* desc, const rrt_attn_weights& lw, const float* xi, float* xo,
                     const Workspace& ws, int64_t N, hipStream_t st) {
  if (!lw.norm2_w || !lw.norm2_b || !lw.fc1_w || !lw.fc1_b || !lw.fc2_w || !lw.fc2_b) return RRT_E_INVALID;
  const int D = desc->dim;
  RRT_TRY(launch_layernorm(xi, nullptr, lw.norm2_w, lw.norm2_b, ws.ffn_ln, (int)N, D, st));
  LinearEpilogue e1{};
  e1.prec = desc->compute;
  e1.bias = lw.fc1_b;
  e1.act = desc->ffn_act;
  RRT_TRY(launch_linear(ws.ffn_ln, lw.fc1_w, ws.ffn_hid, (int)N, desc->ffn_hidden, D, e1, st));
  return (int)launch_linear(ws.ffn_hid, lw.fc2_w, xo, (int)N, D, desc->ffn_hidden,
                            proj_epilogue(lw.fc2_b, xi, identity_grid(N), desc->compute), st);
}

static int encoder_forward(const rrt_encoder_desc* desc_in, const rrt_encoder_weights* w, const float* x,
                           float* y, int64_t n_tokens, void* workspace, size_t workspace_bytes,
                           void* stream, void** events, rrt_phase_gate* gate = nullptr, float* rmsa_out = nullptr,
                           uint16_t* y16 = nullptr, bool* y16_done = nullptr, int rows_w_forced = -1,
                           const float* shortcut = nullptr) {
  // shortcut (rrt_api::encoder_tail): what all_shortcut adds, when it is not this call's x
  // rows_w_forced >= 0 (rrt_debug_encoder_forward_rows_f32): the width of the row-looping K1 / K7 instead of the plan's
  // y16 / y16_done (the slide classifier, 16-bit modes): where the forward's last kernel is CR-MSA's dispatch + LayerNorm it
  // also leaves the output rows as 16-bit values there and sets the flag
  if (y16_done) *y16_done = false;
  if (!desc_in || !w || !x || !y || x == y) return RRT_E_INVALID;
  int rc = check_desc(desc_in, n_tokens);
  if (rc) return rc;
  if (handover_err_peek(false)) return RRT_E_HANDOVER;    // (a host read of pinned memory; rrt_hip.h, rrt_device_error)
  rrt_grid g{}, g8{};
  rc = region_grids(desc_in, n_tokens, &g, &g8);
  if (rc) return rc;
  // RRT_COMPUTE_F32X3 concerns the R-MSA layers' two big projections (plan_encoder); every other GEMM of the call is exact fp32
  rrt_encoder_desc dloc = *desc_in;
  if (dloc.compute == RRT_COMPUTE_F32X3) dloc.compute = RRT_COMPUTE_F32;
  const rrt_encoder_desc* const desc = &dloc;
  hipStream_t st = (hipStream_t)stream;
  const int D = desc->dim;
  const int64_t N = n_tokens;
  Workspace ws = carve(*desc, N, g, g8, nullptr);
  if (!workspace || workspace_bytes < ws.bytes) return RRT_E_WORKSPACE;
  ws = carve(*desc, N, g, g8, (char*)workspace);
  EncoderPlan plan = plan_encoder(*desc_in, g, g8, rmsa_out != nullptr);
  if (rows_w_forced >= 0) {
    plan.rows_w = rows_w_forced;
    plan.rows_ln1 = rows_w_forced > 0 && desc_in->compute == RRT_COMPUTE_F32;
  }

  // optional stage-boundary events (bench.py / profiling): events[i] recorded after stage i-1
  auto mark = [&](int i) -> hipError_t {
    return (events && events[i]) ? hipEventRecord((hipEvent_t)events[i], st) : hipSuccess;
  };
  RRT_TRY(mark(RRT_EV_START));

  auto ffn_block = [&](const rrt_attn_weights& lw, const float* xi, float* xo) -> int {
    return ffn_apply(desc, lw, xi, xo, ws, N, st);
  };

  const float* xin = x;   // current activations [N, D]
  // PEG / PPEG (ablation): before the first layer (pos_pos = -1) or before layer index 1 (pos_pos = 0), rrt.py:181-187
  auto pos_embed = [&]() -> int {
    if (!w->pos_w[0] || (desc->pos == RRT_POS_PPEG && (!w->pos_w[1] || !w->pos_w[2]))) return RRT_E_INVALID;
    RRT_TRY(launch_peg(xin, w->pos_w, w->pos_b, ws.xp, (int)N, D, desc->peg_k, desc->peg_1d, desc->pos == RRT_POS_PPEG, st));
    xin = ws.xp;
    return RRT_OK;
  };
  if (desc->pos && desc->pos_pos == -1) {
    rc = pos_embed();
    if (rc) return rc;
  }
  // The weight images of the reduced-precision / emulated modes (plan.casts: 16-bit copies, or (hi, lo) bf16 pairs = two
  // 16-bit values per weight; plan.inner16: CR-MSA's inner qkv / proj as well) are cast once per call, one launch for all
  // layers, unless the caller vouches for the images already in the workspace (desc.weights16_valid; the ABI keeps no state).
  {
    const bool split = plan.casts == CastKind::Split;
    const size_t per_w = split ? 2 : 1;
    Cast16Jobs jobs{};
    if (plan.casts != CastKind::None) {
      for (int li = 0; li < desc->n_rmsa_layers; ++li) {
        const rrt_attn_weights& lw = w->rmsa[li];
        if (!lw.qkv_w || !lw.proj_w) return RRT_E_INVALID;
        uint16_t* base = ws.w16 + (size_t)li * per_w * 4 * D * D;
        jobs.add(lw.qkv_w, base, (size_t)3 * D * D);
        jobs.add(lw.proj_w, base + per_w * 3 * D * D, (size_t)D * D);
      }
    }
    if (plan.inner16) {
      if (!w->crmsa.qkv_w || !w->crmsa.proj_w) return RRT_E_INVALID;
      jobs.add(w->crmsa.qkv_w, ws.wcr16, (size_t)3 * D * D);
      jobs.add(w->crmsa.proj_w, ws.wcr16 + (size_t)3 * D * D, (size_t)D * D);
    }
    if (jobs.count && !desc->weights16_valid) RRT_TRY(split ? launch_cast_split(jobs, st) : launch_cast16(jobs, desc->compute, st));
  }
  // The phase gate around a layer's MFMA-bound core launch (plan.gated): wait for the previous gated core of any stream, then
  // the LayerNorm-partition mark (it brackets the kernel, not the wait); after the launch, record the gate and mark the core.
  // Marks: layer 0 only, and none for the EPEG ablations.
  rrt_phase_gate* const gt = (gate && plan.gated) ? gate : nullptr;
  auto gate_record = [&]() -> hipError_t {
    if (!gt) return hipSuccess;
    const hipError_t ge = hipEventRecord(gt->done, st);
    if (ge == hipSuccess) gt->armed = true;
    return ge;
  };
  auto core_begin = [&](bool marks) -> hipError_t {
    if (gt && gt->armed) {
      const hipError_t ge = hipStreamWaitEvent(st, gt->done, 0);
      if (ge != hipSuccess) return ge;
    }
    return marks ? mark(RRT_EV_LN_PARTITION) : hipSuccess;
  };
  auto core_end = [&](bool marks, bool record = true) -> hipError_t {
    hipError_t ge = record ? gate_record() : hipSuccess;
    if (ge == hipSuccess && marks) ge = mark(RRT_EV_QKV);
    if (ge == hipSuccess && marks) ge = mark(RRT_EV_ATTN);
    return ge;
  };
  // (tuning build: the two-launch fused kind holds the gate until its out-projection is queued)
  static const bool gate_proj = rrt_tune_env("RRT_GATE_PROJ") != nullptr;
  // ---- R-MSA TransLayers: x = x + unpart(InnerAttention(part(pad(LN(x)))))  (rrt.py:117-125)
  for (int li = 0; li < desc->n_rmsa_layers; ++li) {
    if (li == 1 && desc->pos && desc->pos_pos == 0) {
      rc = pos_embed();
      if (rc) return rc;
    }
    const rrt_attn_weights& lw = w->rmsa[li];
    const bool last = li == desc->n_rmsa_layers - 1;
    if (!lw.norm_w || !lw.norm_b || !lw.qkv_w || !lw.proj_w || !lw.proj_b) return RRT_E_INVALID;
    if (desc->epeg && !lw.pe_w) return RRT_E_INVALID;
    if (plan.parts && last && (!w->crmsa.norm_w || !w->crmsa.norm_b || !w->phi)) return RRT_E_INVALID;
    const GridDev gd = to_dev(g);
    const int R = gd.rs * gd.rs, ek = desc->epeg ? desc->epeg_k : 0;
    const float* const pe_w = desc->epeg ? lw.pe_w : nullptr;
    // without FFN the layers ping-pong xa / xb; with it attention writes xa and the FFN writes xb
    // (rmsa_out: the batch entry point takes the R-MSA layers' result of each bag in its own buffer)
    const bool to_out = rmsa_out != nullptr && last;
    float* xout = desc->ffn ? ws.xa : (to_out ? rmsa_out : ((li & 1) ? ws.xb : ws.xa));
    float* const fout = to_out ? rmsa_out : ws.xb;      // the layer's FFN output
    const bool marks = li == 0 && plan.layer != LayerKind::EpegVariant;
    // the out-projection's epilogue; its side job zeroes the CR-MSA region kernels' arrival counters
    auto out_ep = [&](int prec) {
      LinearEpilogue ep = proj_epilogue(lw.proj_b, xin, gd, prec);
      ep.zero64 = ws.cr_cnt;
      return ep;
    };
    switch (plan.layer) {
      case LayerKind::Pair16Merged:
      case LayerKind::Fused16: {
        // u (16-bit) in the uo buffer, O (16-bit) in the qkv buffer; qkv, scores and probabilities never leave the CU
        const bool merged16 = plan.layer == LayerKind::Pair16Merged;
        uint16_t* u16 = (uint16_t*)ws.uo;
        uint16_t* o16 = (uint16_t*)ws.qkv;
        const uint16_t* wq16 = ws.w16 + (size_t)li * 4 * D * D;
        RRT_TRY(launch_ln_partition16(xin, lw.norm_w, lw.norm_b, u16, D, gd, desc->compute, st, merged16 ? ws.proj_cnt : nullptr,
                                      merged16 ? R / 2 : 0));
        RRT_TRY(core_begin(marks));
        if (merged16) {
          PairProj pj{};
          pj.Wp = wq16 + (size_t)3 * D * D;
          pj.bias = lw.proj_b;
          pj.resid = xin;
          pj.out = xout;
          pj.cnt = ws.proj_cnt;
          pj.zero64 = ws.cr_cnt;
          pj.g = gd;
          RRT_TRY(launch_rmsa_pair16_proj(u16, wq16, lw.qkv_b, pe_w, o16, R, gd.P, D, desc->n_heads, ek, desc->compute, pj, st));
          RRT_TRY(core_end(marks));
        } else {
          RRT_TRY(launch_rmsa_fused16(u16, wq16, lw.qkv_b, pe_w, o16, R, gd.P, D, desc->n_heads, ek, desc->compute, st));
          RRT_TRY(core_end(marks));
          LinearEpilogue ep = out_ep(desc->compute);
          ep.solo = desc->solo != 0;          // (picks the tile shape: one bag in flight / several, launch_linear16)
          RRT_TRY(launch_linear16(o16, wq16 + (size_t)3 * D * D, xout, gd.Np, D, D, ep, st));
        }
        break;
      }
      case LayerKind::FusedX3: {
        // u and O as split images (4 bytes per element: the uo / qkv buffers as they are)
        const uint16_t* wq = ws.w16 + (size_t)li * 8 * D * D;          // 4 D^2 weights x 2 bf16
        RRT_TRY(launch_ln_partition_split(xin, lw.norm_w, lw.norm_b, ws.uo, D, gd, st));
        RRT_TRY(core_begin(marks));
        RRT_TRY(launch_rmsa_fused_x3(ws.uo, wq, lw.qkv_b, pe_w, ws.qkv, R, gd.P, D, desc->n_heads, ek, st));
        RRT_TRY(core_end(marks));
        RRT_TRY(launch_linear_split(ws.qkv, wq + (size_t)6 * D * D, xout, gd.Np, D, D, out_ep(0), st));
        break;
      }
      case LayerKind::FusedProj: {
        // one launch per layer; its arrival counters are zeroed by LayerNorm + partition
        RRT_TRY(launch_ln_partition(xin, lw.norm_w, lw.norm_b, ws.uo, D, gd, st, ws.proj_cnt, R, plan.rows_ln1 ? plan.rows_w : 0));
        RRT_TRY(core_begin(marks));
        FusedProj pj{};
        pj.Wp = lw.proj_w;
        pj.bias = lw.proj_b;
        pj.resid = xin;
        pj.out = xout;
        pj.cnt = ws.proj_cnt;
        pj.zero64 = ws.cr_cnt;
        pj.g = gd;
        // the LAST R-MSA layer feeding CR-MSA directly: its slabs also leave LayerNorm 2's statistics and the logits' dot
        // products of every row (x1 is in their registers), and CR-MSA's first pass shrinks to the combine
        if (plan.parts && last) {
          pj.part = ws.cr_pstat;
          pj.ln_g = w->crmsa.norm_w;
          pj.phi = w->phi;
          pj.k = desc->crmsa_k;
        }
        RRT_TRY(launch_rmsa_fused(ws.uo, lw.qkv_w, lw.qkv_b, pe_w, ws.qkv, R, gd.P, D, desc->n_heads, ek, desc->compute, st,
                                  nullptr, &pj));
        RRT_TRY(core_end(marks));
        break;
      }
      case LayerKind::Fused: {
        // O goes to the qkv workspace (first Np*D floats), u stays in uo
        RRT_TRY(launch_ln_partition(xin, lw.norm_w, lw.norm_b, ws.uo, D, gd, st, nullptr, 0, plan.rows_ln1 ? plan.rows_w : 0));
        RRT_TRY(core_begin(marks));
        RRT_TRY(launch_rmsa_fused(ws.uo, lw.qkv_w, lw.qkv_b, pe_w, ws.qkv, R, gd.P, D, desc->n_heads, ek, desc->compute, st));
        RRT_TRY(core_end(marks, !gate_proj));
        RRT_TRY(launch_linear(ws.qkv, lw.proj_w, xout, gd.Np, D, D, out_ep(desc->compute), st));
        if (gate_proj) RRT_TRY(gate_record());
        break;
      }
      case LayerKind::Unfused: {
        RRT_TRY(launch_ln_partition(xin, lw.norm_w, lw.norm_b, ws.uo, D, gd, st, nullptr, 0, plan.rows_ln1 ? plan.rows_w : 0));
        RRT_TRY(core_begin(marks));
        RRT_TRY(launch_linear(ws.uo, lw.qkv_w, ws.qkv, gd.Np, 3 * D, D, qkv_epilogue(lw.qkv_b, D, desc->n_heads, desc->compute), st));
        if (marks) RRT_TRY(mark(RRT_EV_QKV));
        RRT_TRY(launch_region_attention(ws.qkv, pe_w, ws.uo, R, gd.P, D, desc->n_heads, ek, st));
        if (marks) RRT_TRY(mark(RRT_EV_ATTN));
        RRT_TRY(launch_linear(ws.uo, lw.proj_w, xout, gd.Np, D, D, out_ep(desc->compute), st));
        break;
      }
      case LayerKind::EpegVariant: {
        RRT_TRY(launch_ln_partition(xin, lw.norm_w, lw.norm_b, ws.uo, D, gd, st));
        RRT_TRY(launch_linear(ws.uo, lw.qkv_w, ws.qkv, gd.Np, 3 * D, D, qkv_epilogue(lw.qkv_b, D, desc->n_heads, desc->compute), st));
        if (desc->epeg_type == RRT_EPEG_ATTN) {           // epeg_2d: k x k stencil over the score map
          // (regions of more than ~180 tokens: the score maps live in the workspace instead of the LDS)
          RRT_TRY(launch_attn_scoremap(ws.qkv, lw.pe_w, ws.uo, ws.smap, R, gd.P, D, desc->n_heads, desc->epeg_k, st));
        } else {
          RRT_TRY(launch_value_pe(ws.qkv, lw.pe_w, lw.pe_b, ws.pe_out, R, gd.P, gd.s, D, desc->n_heads, desc->epeg_k,
                                  desc->epeg_2d, st));
          if (desc->epeg_type == RRT_EPEG_VALUE_BF)       // v += pe before attn @ v (rmsa.py:114-118)
            RRT_TRY(launch_add_cols(ws.qkv + 2 * D, ws.pe_out, (size_t)gd.Np, D, 3 * D, st));
          RRT_TRY(launch_region_attention(ws.qkv, nullptr, ws.uo, R, gd.P, D, desc->n_heads, 0, st));
          if (desc->epeg_type == RRT_EPEG_VALUE_AF)       // x += pe after it (rmsa.py:124-129)
            RRT_TRY(launch_add_cols(ws.uo, ws.pe_out, (size_t)gd.Np, D, D, st));
        }
        RRT_TRY(launch_linear(ws.uo, lw.proj_w, xout, gd.Np, D, D, out_ep(desc->compute), st));
        break;
      }
    }
    if (marks) RRT_TRY(mark(RRT_EV_PROJ));
    xin = xout;
    if (desc->ffn) {
      rc = ffn_block(lw, xout, fout);
      if (rc) return rc;
      xin = fout;
    }
  }
  if (rmsa_out != nullptr) {           // batch entry point: stop here, the R-MSA result of this bag in rmsa_out
    if (xin != rmsa_out) RRT_TRY(hipMemcpyAsync(rmsa_out, xin, (size_t)N * D * sizeof(float), hipMemcpyDeviceToDevice, st));
    return RRT_OK;
  }
  const float* x0 = desc->all_shortcut ? (shortcut ? shortcut : x) : nullptr;
  if (!w->norm_w || !w->norm_b) return RRT_E_INVALID;
  if (!desc->cr_msa) {
    RRT_TRY(launch_layernorm(xin, x0, w->norm_w, w->norm_b, y, (int)N, D, st, plan.rows_w));
    RRT_TRY(mark(RRT_EV_END));
    return RRT_OK;
  }
  // ---- CR-MSA TransLayer (rmsa.py:290-337) + all_shortcut + final LayerNorm (rrt.py:190-195)
  const rrt_attn_weights& cw = w->crmsa;
  if (!cw.norm_w || !cw.norm_b || !cw.qkv_w || !cw.proj_w || !cw.proj_b) return RRT_E_INVALID;
  if (desc->crmsa_mlp ? (!w->phi0_w || !w->phi2_w) : !w->phi) return RRT_E_INVALID;
  const GridDev gd8 = to_dev(g8);
  const int k = desc->crmsa_k, R8 = gd8.rs * gd8.rs;
  // every front but Region also leaves the representatives as 16-bit values for the 16-bit inner MSA
  uint16_t* const rep16 = plan.inner16 ? ws.rep16 : nullptr;
  switch (plan.front) {
    case FrontKind::Mlp: {
      // MLP phi (rmsa.py:248-252,305): v = LN(x1) materialised in region-major order, hidden = v W1^T on
      // the matrix cores, logits = tanh(hidden) W2^T; the combine then runs on the normalised rows
      RRT_TRY(launch_ln_partition(xin, cw.norm_w, cw.norm_b, ws.v8, D, gd8, st));
      LinearEpilogue ep{};
      ep.prec = desc->compute;
      RRT_TRY(launch_linear(ws.v8, w->phi0_w, ws.hid, gd8.Np, D / 4, D, ep, st));
      RRT_TRY(launch_crmsa_mlp_logits(ws.hid, w->phi2_w, ws.logits, gd8.Np, D / 4, k, st));
      RRT_TRY(launch_crmsa_combine(ws.v8, nullptr, nullptr, nullptr, ws.logits, ws.wdisp, ws.rep, rep16, desc->compute, D, k, gd8, st));
      break;
    }
    case FrontKind::Parts:
      // LayerNorm 2's statistics and the logits' dot products came out of the projection slabs: one pass over x1, 64 x D / 64
      // independent blocks (crmsa_combine_parts_kernel)
      RRT_TRY(launch_crmsa_combine_parts(xin, ws.cr_pstat, cw.norm_w, cw.norm_b, w->phi, ws.wdisp, ws.rep, rep16, desc->compute, D,
                                         k, gd8, st));
      break;
    case FrontKind::RegionInFlight:
      RRT_TRY(launch_crmsa_region(xin, cw.norm_w, cw.norm_b, w->phi, nullptr, nullptr, ws.wdisp, ws.rep, k, gd8, st, rep16,
                                  desc->compute));
      break;
    case FrontKind::Region4:
      // (its counters were zeroed by this forward's last R-MSA out-projection)
      RRT_TRY(launch_crmsa_region4(xin, cw.norm_w, cw.norm_b, w->phi, nullptr, ws.logits, ws.wdisp, ws.rep, rep16, desc->compute,
                                   ws.cr_part, ws.cr_cnt, k, gd8, st));
      break;
    case FrontKind::Region:
      // logits + combine in one pass over x1 (one block of 16 waves per region, the rows stay in registers)
      RRT_TRY(launch_crmsa_region(xin, cw.norm_w, cw.norm_b, w->phi, nullptr, nullptr, ws.wdisp, ws.rep, k, gd8, st));
      break;
    case FrontKind::Stream4:
      // (counters as Region4's)
      RRT_TRY(launch_crmsa_stream4(xin, cw.norm_w, cw.norm_b, w->phi, nullptr, ws.logits, ws.wdisp, ws.rep, rep16, desc->compute,
                                   ws.cr_part, ws.cr_cnt, k, gd8, st));
      break;
    case FrontKind::TwoKernel:
      RRT_TRY(launch_crmsa_logits(xin, cw.norm_w, cw.norm_b, w->phi, ws.mean_rstd, ws.logits, D, k, gd8, st));
      RRT_TRY(launch_crmsa_combine(xin, cw.norm_w, cw.norm_b, ws.mean_rstd, ws.logits, ws.wdisp, ws.rep, rep16, desc->compute, D, k,
                                   gd8, st));
      break;
    case FrontKind::None: break;      // (cr_msa = 0 and the batch entry point's stop returned above)
  }
  RRT_TRY(mark(RRT_EV_CR_COMBINE));
  // inner MSA over the representatives: batch = k, sequence = R8 regions, no EPEG (rmsa.py:322)
  if (plan.inner16) {
    // reduced-precision modes: qkv projection + attention of the (n, head) pairs as ONE launch of the 16-bit fused R-MSA
    // kernel (k "regions" of 64 tokens, no EPEG), then the out-projection on 16-bit operands
    if (plan.front == FrontKind::Region) {
      Cast16Jobs cj{};
      cj.add(ws.rep, ws.rep16, (size_t)k * R8 * D);
      RRT_TRY(launch_cast16(cj, desc->compute, st));
    }
    RRT_TRY(launch_rmsa_fused16(ws.rep16, ws.wcr16, cw.qkv_b, nullptr, ws.repo16, k, R8, D, desc->crmsa_heads, 0,
                                desc->compute, st));
    LinearEpilogue ep{};
    ep.prec = desc->compute;
    ep.bias = cw.proj_b;
    RRT_TRY(launch_linear16(ws.repo16, ws.wcr16 + (size_t)3 * D * D, ws.rep2, k * R8, D, D, ep, st));
  } else {
    static const bool inner_solo = rrt_tune_env("RRT_INNER_SOLO") != nullptr;     // (A/B: the K-split 16-wave GEMMs also with bags in flight)
    RRT_TRY(inner_attention(ws.rep, k, R8, cw, D, desc->crmsa_heads, 0, ws.rep_qkv, ws.rep_o, desc->compute, desc->solo != 0 || inner_solo, st));
    LinearEpilogue ep{};
    ep.prec = desc->compute;
    ep.bias = cw.proj_b;
    ep.solo = desc->solo != 0 || inner_solo;
    RRT_TRY(launch_linear(ws.rep_o, cw.proj_w, ws.rep2, k * R8, D, D, ep, st));
  }
  RRT_TRY(mark(RRT_EV_CR_INNER));
  if (desc->ffn) {
    // x2 = x1 + dispatch (no LayerNorm yet) -> FFN -> (+ shortcut) -> final LayerNorm.  xin is xb or the
    // caller's x: xa is free for x2, and xin is dead once the dispatch has read it.
    RRT_TRY(launch_crmsa_dispatch_ln(xin, nullptr, ws.wdisp, ws.rep2, nullptr, nullptr, ws.xa, D, k, gd8, st, nullptr, 0, plan.rows_w));
    rc = ffn_block(cw, ws.xa, ws.xb);
    if (rc) return rc;
    RRT_TRY(launch_layernorm(ws.xb, x0, w->norm_w, w->norm_b, y, (int)N, D, st, plan.rows_w));
    RRT_TRY(mark(RRT_EV_END));
    return RRT_OK;
  }
  const bool want16 = y16 != nullptr && (desc->compute == RRT_COMPUTE_BF16 || desc->compute == RRT_COMPUTE_F16) && D % 4 == 0;
  RRT_TRY(launch_crmsa_dispatch_ln(xin, x0, ws.wdisp, ws.rep2, w->norm_w, w->norm_b, y, D, k,
                                   gd8, st, want16 ? y16 : nullptr, want16 ? desc->compute : 0, plan.rows_w));
  if (want16 && y16_done) *y16_done = true;
  RRT_TRY(mark(RRT_EV_END));
  return RRT_OK;
}

int rrt_encoder_forward_f32(const rrt_encoder_desc* desc, const rrt_encoder_weights* w, const float* x,
                            float* y, int64_t n_tokens, void* workspace, size_t workspace_bytes,
                            void* stream) {
  return encoder_forward(desc, w, x, y, n_tokens, workspace, workspace_bytes, stream, nullptr);
}

int rrt_debug_encoder_forward_rows_f32(const rrt_encoder_desc* desc, const rrt_encoder_weights* w, const float* x, float* y,
                                       int64_t n_tokens, void* workspace, size_t workspace_bytes, void* stream, int32_t rows_w) {
  if (rows_w < 0 || rows_w > ROWS_W_MAX) return RRT_E_INVALID;
  return encoder_forward(desc, w, x, y, n_tokens, workspace, workspace_bytes, stream, nullptr, nullptr, nullptr, nullptr, nullptr,
                         rows_w);
}

}  // extern "C"

// what api_nystrom.hip composes its encoder forward on (api_internal.h): the forward without attention layers and without
// PEG / PPEG, on a copy of the descriptor
namespace rrt_api {
static rrt_encoder_desc tail_desc(const rrt_encoder_desc* desc) {
  rrt_encoder_desc t = *desc;
  t.n_rmsa_layers = 0;
  t.pos = RRT_POS_NONE;
  t.weights16_valid = 0;
  return t;
}
int encoder_tail_workspace_size(const rrt_encoder_desc* desc, int64_t n_tokens, size_t* bytes) {
  const rrt_encoder_desc t = tail_desc(desc);
  return rrt_encoder_workspace_size(&t, n_tokens, bytes);
}
int encoder_tail(const rrt_encoder_desc* desc, const rrt_encoder_weights* w, const float* x1, const float* x0, float* y,
                 int64_t n_tokens, void* workspace, size_t workspace_bytes, void* stream) {
  const rrt_encoder_desc t = tail_desc(desc);
  return encoder_forward(&t, w, x1, y, n_tokens, workspace, workspace_bytes, stream, nullptr, nullptr, nullptr, nullptr, nullptr,
                         -1, x0);
}
}  // namespace rrt_api

extern "C" {
int rrt_phase_gate_create(rrt_phase_gate** out) {
  if (!out) return RRT_E_INVALID;
  rrt_phase_gate* g = new rrt_phase_gate();
  g->armed = false;
  hipError_t e = hipEventCreateWithFlags(&g->done, hipEventDisableTiming);
  if (e != hipSuccess) {
    delete g;
    return (int)e;
  }
  *out = g;
  return RRT_OK;
}

int rrt_phase_gate_destroy(rrt_phase_gate* g) {
  if (!g) return RRT_OK;
  (void)hipEventDestroy(g->done);
  delete g;
  return RRT_OK;
}

int rrt_encoder_forward_gated_f32(const rrt_encoder_desc* desc, const rrt_encoder_weights* w, const float* x,
                                  float* y, int64_t n_tokens, void* workspace, size_t workspace_bytes,
                                  void* stream, rrt_phase_gate* gate, void** events) {
  return encoder_forward(desc, w, x, y, n_tokens, workspace, workspace_bytes, stream, events, gate);
}

int rrt_encoder_forward_events_f32(const rrt_encoder_desc* desc, const rrt_encoder_weights* w,
                                   const float* x, float* y, int64_t n_tokens, void* workspace,
                                   size_t workspace_bytes, void* stream, void** events) {
  return encoder_forward(desc, w, x, y, n_tokens, workspace, workspace_bytes, stream, events);
}

// ---- batch > 1 (modules/rrt.py:165-202 on (B, N, D) input).  The reference's region_partition puts the regions of all
// bags of the batch on one leading axis (rmsa.py:28-39), so the R-MSA layers treat the bags independently, but CR-MSA's
// inner attention runs over the 64 B representatives of ALL bags (rmsa.py:316-322: batch = k, sequence = B * 64): the bags
// are coupled there and only there.  Here: the R-MSA layers bag by bag (the single-bag path, results in x1 [B, N, D]),
// statistics + combine per bag into rep [k, 64 B, D] (region b * 64 + w), ONE inner MSA over sequences of 64 B tokens, the
// dispatch + final LayerNorm per bag.  Correctness path for the literal drop-in contract (every reference trainer uses
// B = 1): the chip-wide two-kernel statistics / combine and the generic attention kernel, fp32 data; inference only.
namespace {
struct BatchWs {
  Workspace one;          // the single-bag workspace (R-MSA layers, FFN / MLP-phi temporaries), reused bag after bag
  float *x1, *mean_rstd, *logits, *wdisp, *rep, *rep_qkv, *rep_o, *rep2;
  size_t one_bytes, bytes;
};
BatchWs carve_batch(const rrt_encoder_desc& d, int64_t B, int64_t N, const rrt_grid& g, const rrt_grid& g8, char* base) {
  BatchWs w{};
  // (the single-bag carve is sized by its QUERY form: with ffn = 1 the query counts xa / xb twice -- a null pointer does not
  //  tell it they are taken -- so the queried size, which encoder_forward checks against, exceeds what the real carve uses)
  w.one_bytes = carve(d, N, g, g8, nullptr).bytes;
  Arena a{base};
  w.one = carve(d, N, g, g8, a.take<char>(w.one_bytes));
  const size_t D = d.dim, Np8 = (size_t)g8.H * g8.H, R8 = (size_t)g8.regions_side * g8.regions_side, k = d.crmsa_k;
  w.x1 = a.take((size_t)B * N * D);
  if (d.cr_msa) {
    w.mean_rstd = a.take((size_t)B * N * 2);
    w.logits = a.take((size_t)B * Np8 * k);
    w.wdisp = a.take((size_t)B * Np8 * k);
    w.rep = a.take(k * R8 * B * D);
    w.rep_qkv = a.take(k * R8 * B * 3 * D);
    w.rep_o = a.take(k * R8 * B * D);
    w.rep2 = a.take(k * R8 * B * D);
  }
  w.bytes = a.bytes();
  return w;
}
}  // namespace

int rrt_encoder_batch_workspace_size(const rrt_encoder_desc* desc, int32_t batch, int64_t n_tokens, size_t* bytes) {
  if (!bytes || batch <= 0) return RRT_E_INVALID;
  rrt_grid g{}, g8{};
  int rc = resolve_grids(desc, n_tokens, &g, &g8);
  if (rc) return rc;
  *bytes = carve_batch(*desc, batch, n_tokens, g, g8, nullptr).bytes;
  return RRT_OK;
}

int rrt_encoder_forward_batch_f32(const rrt_encoder_desc* desc_in, const rrt_encoder_weights* w, const float* x, float* y,
                                  int32_t batch, int64_t n_tokens, void* workspace, size_t workspace_bytes, void* stream) {
  if (!desc_in || !w || !x || !y || x == y || batch <= 0) return RRT_E_INVALID;
  int rc = check_desc(desc_in, n_tokens);
  if (rc) return rc;
  if (batch > 1024) return unsupported("batch > 1024");
  rrt_encoder_desc dloc = *desc_in;
  dloc.weights16_valid = 0;     // (the first bag writes the images; the later bags of THIS call may reuse them, below)
  dloc.solo = 0;
  const rrt_encoder_desc* const desc = &dloc;
  const int64_t N = n_tokens, B = batch;
  const int D = desc->dim;
  hipStream_t st = (hipStream_t)stream;
  rrt_grid g{}, g8{};
  rc = region_grids(desc, N, &g, &g8);
  if (rc) return rc;
  BatchWs bw = carve_batch(*desc, B, N, g, g8, nullptr);
  if (!workspace || workspace_bytes < bw.bytes) return RRT_E_WORKSPACE;
  bw = carve_batch(*desc, B, N, g, g8, (char*)workspace);
  // ---- positional encoder + R-MSA layers, bag by bag -> x1 [B, N, D]
  for (int64_t b = 0; b < B; ++b) {
    rc = encoder_forward(&dloc, w, x + (size_t)b * N * D, y + (size_t)b * N * D, N, workspace, bw.one_bytes, stream, nullptr,
                         nullptr, bw.x1 + (size_t)b * N * D);
    if (rc) return rc;
    dloc.weights16_valid = 1;   // same workspace, same weights, same mode: the images of bag 0 stand
  }
  dloc.weights16_valid = 0;
  if (!w->norm_w || !w->norm_b) return RRT_E_INVALID;
  if (!desc->cr_msa) {
    for (int64_t b = 0; b < B; ++b)
      RRT_TRY(launch_layernorm(bw.x1 + (size_t)b * N * D, desc->all_shortcut ? x + (size_t)b * N * D : nullptr, w->norm_w,
                               w->norm_b, y + (size_t)b * N * D, (int)N, D, st));
    return RRT_OK;
  }
  // ---- CR-MSA over the batch (rmsa.py:290-337)
  const rrt_attn_weights& cw = w->crmsa;
  if (!cw.norm_w || !cw.norm_b || !cw.qkv_w || !cw.proj_w || !cw.proj_b) return RRT_E_INVALID;
  if (desc->crmsa_mlp ? (!w->phi0_w || !w->phi2_w) : !w->phi) return RRT_E_INVALID;
  GridDev gd8 = to_dev(g8);
  const int k = desc->crmsa_k, R8 = gd8.rs * gd8.rs;
  gd8.Rt = R8 * (int)B;                                  // rep / rep2 rows: [k][B * R8]
  const size_t Np8 = (size_t)gd8.Np;
  // (F32X3 concerns the R-MSA projections only; CR-MSA's GEMMs round their operands in the bf16 / fp16 modes)
  const int prec = desc->compute == RRT_COMPUTE_F32X3 ? RRT_COMPUTE_F32 : desc->compute;
  for (int64_t b = 0; b < B; ++b) {
    const float* xb1 = bw.x1 + (size_t)b * N * D;
    float* lg = bw.logits + (size_t)b * Np8 * k;
    float* wd = bw.wdisp + (size_t)b * Np8 * k;
    float* repb = bw.rep + (size_t)b * R8 * D;          // region 0 of bag b in every representative's row
    if (desc->crmsa_mlp) {
      RRT_TRY(launch_ln_partition(xb1, cw.norm_w, cw.norm_b, bw.one.v8, D, gd8, st));
      LinearEpilogue ep{};
      ep.prec = prec;
      RRT_TRY(launch_linear(bw.one.v8, w->phi0_w, bw.one.hid, gd8.Np, D / 4, D, ep, st));
      RRT_TRY(launch_crmsa_mlp_logits(bw.one.hid, w->phi2_w, lg, gd8.Np, D / 4, k, st));
      RRT_TRY(launch_crmsa_combine(bw.one.v8, nullptr, nullptr, nullptr, lg, wd, repb, nullptr, 0, D, k, gd8, st));
    } else {
      float* mr = bw.mean_rstd + (size_t)b * N * 2;
      RRT_TRY(launch_crmsa_logits(xb1, cw.norm_w, cw.norm_b, w->phi, mr, lg, D, k, gd8, st));
      RRT_TRY(launch_crmsa_combine(xb1, cw.norm_w, cw.norm_b, mr, lg, wd, repb, nullptr, 0, D, k, gd8, st));
    }
  }
  // inner MSA: batch = k, sequence = the B * R8 representatives of all bags, no EPEG (rmsa.py:322)
  RRT_TRY(inner_attention(bw.rep, k, R8 * (int)B, cw, D, desc->crmsa_heads, 0, bw.rep_qkv, bw.rep_o, prec, false, st));
  {
    LinearEpilogue ep{};
    ep.prec = prec;
    ep.bias = cw.proj_b;
    RRT_TRY(launch_linear(bw.rep_o, cw.proj_w, bw.rep2, k * R8 * (int)B, D, D, ep, st));
  }
  for (int64_t b = 0; b < B; ++b) {
    const float* xb1 = bw.x1 + (size_t)b * N * D;
    const float* x0 = desc->all_shortcut ? x + (size_t)b * N * D : nullptr;
    const float* wd = bw.wdisp + (size_t)b * Np8 * k;
    const float* rep2b = bw.rep2 + (size_t)b * R8 * D;
    float* yb = y + (size_t)b * N * D;
    if (desc->ffn) {
      // x2 = x1 + dispatch (no LayerNorm yet) -> FFN -> (+ shortcut) -> final LayerNorm
      RRT_TRY(launch_crmsa_dispatch_ln(xb1, nullptr, wd, rep2b, nullptr, nullptr, bw.one.xa, D, k, gd8, st));
      rc = ffn_apply(desc, cw, bw.one.xa, bw.one.xb, bw.one, N, st);
      if (rc) return rc;
      RRT_TRY(launch_layernorm(bw.one.xb, x0, w->norm_w, w->norm_b, yb, (int)N, D, st));
    } else {
      RRT_TRY(launch_crmsa_dispatch_ln(xb1, x0, wd, rep2b, w->norm_w, w->norm_b, yb, D, k, gd8, st));
    }
  }
  return RRT_OK;
}

// ------------------------------------------------------------------ stage entry points
int rrt_ln_partition_f32(const float* x, const float* gamma, const float* beta, float* u, int64_t L,
                         int32_t dim, const rrt_grid* g, void* stream) {
  if (!x || !gamma || !beta || !u || !g || L != g->L || dim <= 0 || dim % 4) return RRT_E_INVALID;
  if (dim > 2048) return unsupported("dim > 2048");
  return (int)launch_ln_partition(x, gamma, beta, u, dim, to_dev(*g), (hipStream_t)stream);
}

int rrt_ln_partition_rows_f32(const float* x, const float* gamma, const float* beta, float* u, int64_t L,
                              int32_t dim, const rrt_grid* g, int32_t w, int32_t* zero, int32_t n_zero, void* stream) {
  if (!x || !gamma || !beta || !u || !g || L != g->L || dim <= 0 || dim % 4) return RRT_E_INVALID;
  if (w < 0 || w > ROWS_W_MAX || n_zero < 0 || (n_zero > 0 && !zero)) return RRT_E_INVALID;
  if (dim > 2048) return unsupported("dim > 2048");
  return (int)launch_ln_partition(x, gamma, beta, u, dim, to_dev(*g), (hipStream_t)stream, n_zero > 0 ? zero : nullptr, n_zero, w);
}

int rrt_linear_f32(const float* A, const float* B, const float* bias, float* C, int64_t M, int32_t N,
                   int32_t K, int32_t q_cols, float q_scale, int32_t compute, void* stream) {
  if (!A || !B || !C || M <= 0 || N <= 0 || K <= 0) return RRT_E_INVALID;
  if (K % 32) return unsupported("linear: K must be a multiple of 32");
  if (compute < 0 || compute > 2) return unsupported("compute must be RRT_COMPUTE_F32/BF16/F16");
  LinearEpilogue ep{};
  ep.prec = compute;
  ep.bias = bias;
  ep.q_cols = q_cols;
  ep.q_scale = q_scale;
  return (int)launch_linear(A, B, C, (int)M, N, K, ep, (hipStream_t)stream);
}

int rrt_linear_unpartition_residual_f32(const float* A, const float* B, const float* bias,
                                        const float* resid, float* out, int32_t N, int32_t K,
                                        const rrt_grid* g, int32_t compute, void* stream) {
  if (!A || !B || !resid || !out || !g || N <= 0 || K <= 0) return RRT_E_INVALID;
  if (K % 32) return unsupported("linear: K must be a multiple of 32");
  if (compute < 0 || compute > 2) return unsupported("compute must be RRT_COMPUTE_F32/BF16/F16");
  const LinearEpilogue ep = proj_epilogue(bias, resid, to_dev(*g), compute);
  return (int)launch_linear(A, B, out, ep.g.Np, N, K, ep, (hipStream_t)stream);
}

int rrt_region_attention_f32(const float* qkv, const float* pe_w, float* o, int32_t n_regions, int32_t P,
                             int32_t dim, int32_t heads, int32_t epeg_k, void* stream) {
  if (!qkv || !o || n_regions <= 0 || P <= 0 || dim <= 0 || heads <= 0 || dim % heads) return RRT_E_INVALID;
  if (pe_w && epeg_k > 0 && epeg_k % 2 == 0) return unsupported("epeg_k must be odd");
  return (int)launch_region_attention(qkv, pe_w, o, n_regions, P, dim, heads, epeg_k, (hipStream_t)stream);
}

int rrt_region_attention_hd_supported(int32_t P, int32_t dim, int32_t heads, int32_t epeg_k) {
  return region_attention_hd_supported(P, dim, heads, epeg_k) ? 1 : 0;
}

int rrt_region_attention_hd_f32(const float* qkv, const float* pe_w, float* o, int32_t n_regions, int32_t P, int32_t dim,
                                int32_t heads, int32_t epeg_k, void* stream) {
  if (n_regions <= 0 || P <= 0 || dim <= 0 || heads <= 0 || dim % heads) return RRT_E_INVALID;
  const int ek = pe_w ? epeg_k : 0;
  if (!region_attention_hd_supported(P, dim, heads, ek))      // before the pointers: nothing is touched outside the predicate
    return unsupported("region_attention_hd: needs a head dim that is a multiple of 16 in [16, 256] other than 64 and "
                       "epeg_k <= 63 (use rrt_region_attention_f32)");
  if (!qkv || !o) return RRT_E_INVALID;
  if (ek > 0 && ek % 2 == 0) return unsupported("epeg_k must be odd");
  if (n_regions > 65535) return unsupported("region_attention_hd: more than 65535 regions in one call");
  return (int)launch_region_attention_hd(qkv, pe_w, o, n_regions, P, dim, heads, ek, (hipStream_t)stream);
}

int rrt_rmsa_fused_f32(const float* u, const float* qkv_w, const float* qkv_b, const float* pe_w, float* o,
                       int32_t n_regions, int32_t P, int32_t dim, int32_t heads, int32_t epeg_k,
                       int32_t compute, void* stream) {
  if (!u || !qkv_w || !o || n_regions <= 0 || P <= 0 || dim <= 0 || heads <= 0) return RRT_E_INVALID;
  if (compute < 0 || compute > 2) return unsupported("compute must be RRT_COMPUTE_F32/BF16/F16");
  const int ek = pe_w ? epeg_k : 0;
  if (!rmsa_fused_supported(P, dim, heads, ek) || !rmsa_fused_supported_rows((long)n_regions * P, dim))
    return unsupported("rmsa_fused: needs head dim 64, 48 < P <= 208, epeg_k <= 63 (use linear + region_attention)");
  return (int)launch_rmsa_fused(u, qkv_w, qkv_b, pe_w, o, n_regions, P, dim, heads, ek, compute,
                                (hipStream_t)stream);
}

int rrt_device_error(int32_t clear) { return handover_err_peek(clear != 0); }

int rrt_rmsa_fused_proj_f32(const float* u, const float* qkv_w, const float* qkv_b, const float* pe_w,
                            const float* proj_w, const float* proj_b, const float* resid, float* out, float* o_scratch,
                            int32_t* counters, int32_t dim, int32_t heads, int32_t epeg_k, const rrt_grid* g,
                            void* stream) {
  return rrt_debug_rmsa_fused_proj_f32(u, qkv_w, qkv_b, pe_w, proj_w, proj_b, resid, out, o_scratch, counters, dim, heads,
                                       epeg_k, g, 0, 0, 0, stream);
}

}  // extern "C"

// the merged launch of one layer through the stage entry points (tests): optional test knobs, optional CR-MSA row records
static int fused_proj_stage(const float* u, const float* qkv_w, const float* qkv_b, const float* pe_w,
                            const float* proj_w, const float* proj_b, const float* resid, float* out, float* o_scratch,
                            int32_t* counters, int32_t dim, int32_t heads, int32_t epeg_k, const rrt_grid* g,
                            int32_t lag, int32_t spin_limit, int32_t wait_extra, const float* ln2_gamma, const float* phi,
                            int32_t crmsa_k, float* part, void* stream) {
  if (!u || !qkv_w || !proj_w || !resid || !out || !o_scratch || !counters || !g || dim <= 0 || heads <= 0 || out == resid ||
      lag < 0 || spin_limit < 0 || wait_extra < 0)
    return RRT_E_INVALID;
  if (handover_err_peek(false)) return RRT_E_HANDOVER;
  const GridDev gd = to_dev(*g);
  const int ek = pe_w ? epeg_k : 0, R = gd.rs * gd.rs;
  if (!rmsa_fused_proj_supported(R, gd.P, dim, heads, ek, RRT_COMPUTE_F32) || !rmsa_fused_supported_rows(gd.Np, dim))
    return unsupported("rmsa_fused_proj: needs what rmsa_fused needs (head dim 64, 64 < P <= 208, epeg_k <= 63) and at "
                       "least two rounds of (region, head) items (heads * regions >= 2 x the CU count)");
  RRT_TRY(hipMemsetAsync(counters, 0, (size_t)R * sizeof(int32_t), (hipStream_t)stream));
  FusedProj pj{};
  pj.Wp = proj_w;
  pj.bias = proj_b;
  pj.resid = resid;
  pj.out = out;
  pj.cnt = counters;
  pj.g = gd;
  pj.lag = lag;
  pj.spin_limit = spin_limit;
  pj.wait_for = wait_extra > 0 ? heads + wait_extra : 0;
  pj.part = part;
  pj.ln_g = ln2_gamma;
  pj.phi = phi;
  pj.k = crmsa_k;
  if (lag > 0 && (lag < 8 * heads || lag > heads * R)) return unsupported("rmsa_fused_proj: lag must be in [8 * heads, heads * regions]");
  return (int)launch_rmsa_fused(u, qkv_w, qkv_b, pe_w, o_scratch, R, gd.P, dim, heads, ek, RRT_COMPUTE_F32,
                                (hipStream_t)stream, nullptr, &pj);
}

extern "C" {

int rrt_debug_rmsa_fused_proj_f32(const float* u, const float* qkv_w, const float* qkv_b, const float* pe_w,
                                  const float* proj_w, const float* proj_b, const float* resid, float* out, float* o_scratch,
                                  int32_t* counters, int32_t dim, int32_t heads, int32_t epeg_k, const rrt_grid* g,
                                  int32_t lag, int32_t spin_limit, int32_t wait_extra, void* stream) {
  return fused_proj_stage(u, qkv_w, qkv_b, pe_w, proj_w, proj_b, resid, out, o_scratch, counters, dim, heads, epeg_k, g, lag,
                          spin_limit, wait_extra, nullptr, nullptr, 0, nullptr, stream);
}

int rrt_rmsa_fused_proj_stats_f32(const float* u, const float* qkv_w, const float* qkv_b, const float* pe_w,
                                  const float* proj_w, const float* proj_b, const float* resid, float* out, float* o_scratch,
                                  int32_t* counters, const float* ln2_gamma, const float* phi, int32_t crmsa_k, float* part,
                                  int32_t dim, int32_t heads, int32_t epeg_k, const rrt_grid* g, void* stream) {
  if (!ln2_gamma || !phi || !part || crmsa_k < 1 || crmsa_k > RRT_MAX_CRMSA_K) return RRT_E_INVALID;
  return fused_proj_stage(u, qkv_w, qkv_b, pe_w, proj_w, proj_b, resid, out, o_scratch, counters, dim, heads, epeg_k, g, 0, 0, 0,
                          ln2_gamma, phi, crmsa_k, part, stream);
}

int rrt_crmsa_combine_parts_f32(const float* x1, const float* part, const float* gamma, const float* beta, const float* phi,
                                float* wdisp, float* rep, int64_t n_tokens, int32_t dim, int32_t k, const rrt_grid* g8,
                                void* stream) {
  if (!x1 || !part || !gamma || !beta || !phi || !wdisp || !rep || !g8 || n_tokens <= 0 || g8->L != n_tokens) return RRT_E_INVALID;
  const GridDev gd = to_dev(*g8);
  if (!crmsa_combine_parts_supported(dim, k, gd)) return unsupported("crmsa_combine_parts: dim % 64 == 0, dim <= 512, 1 <= k <= 8");
  return (int)launch_crmsa_combine_parts(x1, part, gamma, beta, phi, wdisp, rep, nullptr, 0, dim, k, gd, (hipStream_t)stream);
}

// ---- 16-bit operand stages of the reduced-precision modes (cast16.hip, linear_f32.hip IN16, rmsa_fused16.hip)
int rrt_cast16(const float* src, uint16_t* dst, int64_t n, int32_t compute, void* stream) {
  if (!src || !dst || n <= 0 || n % 4) return RRT_E_INVALID;
  if (compute != RRT_COMPUTE_BF16 && compute != RRT_COMPUTE_F16) return unsupported("cast16: compute must be BF16 or F16");
  Cast16Jobs jobs{};
  jobs.add(src, dst, (size_t)n);
  return (int)launch_cast16(jobs, compute, (hipStream_t)stream);
}

int rrt_ln_partition16(const float* x, const float* gamma, const float* beta, uint16_t* u, int64_t L, int32_t dim,
                       const rrt_grid* g, int32_t compute, void* stream) {
  if (!x || !gamma || !beta || !u || !g || L != g->L || dim <= 0 || dim % 4) return RRT_E_INVALID;
  if (dim > 2048) return unsupported("dim > 2048");
  if (compute != RRT_COMPUTE_BF16 && compute != RRT_COMPUTE_F16) return unsupported("compute must be BF16 or F16");
  return (int)launch_ln_partition16(x, gamma, beta, u, dim, to_dev(*g), compute, (hipStream_t)stream);
}

int rrt_linear16_f32(const uint16_t* A, const uint16_t* B, const float* bias, const float* resid, float* C, int64_t M,
                     int32_t N, int32_t K, const rrt_grid* g, int32_t compute, void* stream) {
  if (!A || !B || !C || M <= 0 || N <= 0 || K <= 0 || (resid && !g)) return RRT_E_INVALID;
  if (K % 64) return unsupported("linear16: K must be a multiple of 64");
  if (compute != RRT_COMPUTE_BF16 && compute != RRT_COMPUTE_F16) return unsupported("compute must be BF16 or F16");
  LinearEpilogue ep{};
  ep.prec = compute;
  ep.bias = bias;
  if (resid) {
    ep.resid = resid;
    ep.g = to_dev(*g);
    if (M != ep.g.Np) return RRT_E_INVALID;
  }
  return (int)launch_linear16(A, B, C, (int)M, N, K, ep, (hipStream_t)stream);
}

int rrt_rmsa_fused16(const uint16_t* u, const uint16_t* qkv_w, const float* qkv_b, const float* pe_w, uint16_t* o,
                     int32_t n_regions, int32_t P, int32_t dim, int32_t heads, int32_t epeg_k, int32_t compute,
                     void* stream) {
  if (!u || !qkv_w || !o || n_regions <= 0 || P <= 0 || dim <= 0 || heads <= 0) return RRT_E_INVALID;
  if (compute != RRT_COMPUTE_BF16 && compute != RRT_COMPUTE_F16) return unsupported("compute must be BF16 or F16");
  const int ek = pe_w ? epeg_k : 0;
  if (!rmsa_fused16_supported(P, dim, heads, ek) || !rmsa_fused_supported_rows((long)n_regions * P, dim))
    return unsupported("rmsa_fused16: needs head dim 64, 16 < P <= 256, epeg_k <= 63");
  return (int)launch_rmsa_fused16(u, qkv_w, qkv_b, pe_w, o, n_regions, P, dim, heads, ek, compute, (hipStream_t)stream);
}

int rrt_rmsa_pair16_proj(const uint16_t* u, const uint16_t* qkv_w, const float* qkv_b, const float* pe_w, const uint16_t* proj_w,
                         const float* proj_b, const float* resid, float* out, uint16_t* o, int32_t* cnt, int32_t dim,
                         int32_t heads, int32_t epeg_k, const rrt_grid* g, int32_t compute, void* stream) {
  if (!u || !qkv_w || !proj_w || !resid || !out || !o || !cnt || !g || dim <= 0 || heads <= 0) return RRT_E_INVALID;
  if (compute != RRT_COMPUTE_BF16 && compute != RRT_COMPUTE_F16) return unsupported("compute must be BF16 or F16");
  if (handover_err_peek(false)) return RRT_E_HANDOVER;
  const GridDev gd = to_dev(*g);
  const int ek = pe_w ? epeg_k : 0, R = gd.rs * gd.rs;
  if (!rmsa_pair16_proj_supported(R, gd.P, dim, heads, ek))
    return unsupported("rmsa_pair16_proj: head dim 64, regions of 65..96 or 113..128 tokens, a multiple of 16 regions, "
                       "at least two rounds of (pair, head) items");
  RRT_TRY(hipMemsetAsync(cnt, 0, (size_t)(R / 2) * sizeof(int), (hipStream_t)stream));
  PairProj pj{};
  pj.Wp = proj_w;
  pj.bias = proj_b;
  pj.resid = resid;
  pj.out = out;
  pj.cnt = cnt;
  pj.g = gd;
  return (int)launch_rmsa_pair16_proj(u, qkv_w, qkv_b, pe_w, o, R, gd.P, dim, heads, ek, compute, pj, (hipStream_t)stream);
}

// ---- RRT_COMPUTE_F32X3 stages: fp32 as (hi, lo) bf16 pairs (cast16.hip), three bf16 MFMAs per product
int rrt_cast_split(const float* src, void* dst, int64_t n, void* stream) {
  if (!src || !dst || n <= 0 || n % 32) return RRT_E_INVALID;
  Cast16Jobs jobs{};
  jobs.add(src, (uint16_t*)dst, (size_t)n);
  return (int)launch_cast_split(jobs, (hipStream_t)stream);
}

int rrt_ln_partition_split(const float* x, const float* gamma, const float* beta, void* u, int64_t L, int32_t dim,
                           const rrt_grid* g, void* stream) {
  if (!x || !gamma || !beta || !u || !g || L != g->L || dim <= 0 || dim % 32) return RRT_E_INVALID;
  if (dim > 2048) return unsupported("dim > 2048");
  return (int)launch_ln_partition_split(x, gamma, beta, u, dim, to_dev(*g), (hipStream_t)stream);
}

int rrt_linear_split_f32(const void* A, const void* B, const float* bias, const float* resid, float* C, int64_t M,
                         int32_t N, int32_t K, const rrt_grid* g, void* stream) {
  if (!A || !B || !C || M <= 0 || N <= 0 || K <= 0 || (resid && !g)) return RRT_E_INVALID;
  if (K % 32) return unsupported("linear_split: K must be a multiple of 32");
  LinearEpilogue ep{};
  ep.bias = bias;
  if (resid) {
    ep.resid = resid;
    ep.g = to_dev(*g);
    if (M != ep.g.Np) return RRT_E_INVALID;
  }
  return (int)launch_linear_split(A, B, C, (int)M, N, K, ep, (hipStream_t)stream);
}

int rrt_rmsa_fused_x3(const void* u, const void* qkv_w, const float* qkv_b, const float* pe_w, void* o,
                      int32_t n_regions, int32_t P, int32_t dim, int32_t heads, int32_t epeg_k, void* stream) {
  if (!u || !qkv_w || !o || n_regions <= 0 || P <= 0 || dim <= 0 || heads <= 0) return RRT_E_INVALID;
  const int ek = pe_w ? epeg_k : 0;
  if (!rmsa_fused_x3_supported(P, dim, heads, ek) || !rmsa_fused_supported_rows((long)n_regions * P, dim))
    return unsupported("rmsa_fused_x3: needs head dim 64, 48 < P <= 144, epeg_k <= 63");
  return (int)launch_rmsa_fused_x3(u, qkv_w, qkv_b, pe_w, o, n_regions, P, dim, heads, ek, (hipStream_t)stream);
}

int rrt_crmsa_logits_f32(const float* x1, const float* gamma, const float* beta, const float* phi,
                         float* mean_rstd, float* logits, int64_t L, int32_t dim, int32_t k,
                         const rrt_grid* g8, void* stream) {
  if (!x1 || !gamma || !beta || !phi || !mean_rstd || !logits || !g8 || L != g8->L) return RRT_E_INVALID;
  if (k <= 0 || k > RRT_MAX_CRMSA_K || dim % 4 || dim > 2048) return unsupported("crmsa: k in [1,8], dim%4==0, dim<=2048");
  return (int)launch_crmsa_logits(x1, gamma, beta, phi, mean_rstd, logits, dim, k, to_dev(*g8),
                                  (hipStream_t)stream);
}

int rrt_crmsa_combine_f32(const float* x1, const float* gamma, const float* beta, const float* mean_rstd,
                          const float* logits, float* wdisp, float* rep, int64_t L, int32_t dim, int32_t k,
                          const rrt_grid* g8, void* stream) {
  if (!x1 || !logits || !wdisp || !rep || !g8 || L != g8->L) return RRT_E_INVALID;
  if (mean_rstd && (!gamma || !beta)) return RRT_E_INVALID;
  if (k <= 0 || k > RRT_MAX_CRMSA_K || dim % 4) return unsupported("crmsa: k in [1,8], dim%4==0");
  return (int)launch_crmsa_combine(x1, gamma, beta, mean_rstd, logits, wdisp, rep, nullptr, 0, dim, k, to_dev(*g8),
                                   (hipStream_t)stream);
}

int rrt_crmsa_region_f32(const float* x1, const float* gamma, const float* beta, const float* phi, float* mean_rstd,
                         float* logits, float* wdisp, float* rep, int64_t L, int32_t dim, int32_t k, const rrt_grid* g8,
                         void* stream) {
  if (!x1 || !gamma || !beta || !phi || !wdisp || !rep || !g8 || L != g8->L) return RRT_E_INVALID;
  const GridDev gd = to_dev(*g8);
  if (!crmsa_region_supported(dim, k, gd)) return unsupported("crmsa_region: dim = 512, k <= 3, regions of <= 144 tokens");
  return (int)launch_crmsa_region(x1, gamma, beta, phi, mean_rstd, logits, wdisp, rep, k, gd, (hipStream_t)stream);
}

int rrt_crmsa_region4_f32(const float* x1, const float* gamma, const float* beta, const float* phi, float* mean_rstd,
                          float* logits, float* wdisp, float* rep, int64_t L, int32_t dim, int32_t k, const rrt_grid* g8,
                          void* scratch, size_t scratch_bytes, void* stream) {
  if (!x1 || !gamma || !beta || !phi || !logits || !wdisp || !rep || !g8 || !scratch || L != g8->L) return RRT_E_INVALID;
  const GridDev gd = to_dev(*g8);
  if (!crmsa_region4_supported(dim, k, gd)) return unsupported("crmsa_region4: dim = 512, k <= 8, regions of 4..576 tokens");
  if (scratch_bytes < 256 + crmsa_region4_scratch_floats(gd, k) * sizeof(float)) return RRT_E_WORKSPACE;
  RRT_TRY(hipMemsetAsync(scratch, 0, 256, (hipStream_t)stream));      // the arrival counters
  return (int)launch_crmsa_region4(x1, gamma, beta, phi, mean_rstd, logits, wdisp, rep, nullptr, 0,
                                   (float*)((char*)scratch + 256), (int*)scratch, k, gd, (hipStream_t)stream);
}

int rrt_crmsa_stream4_f32(const float* x1, const float* gamma, const float* beta, const float* phi, float* mean_rstd,
                          float* logits, float* wdisp, float* rep, int64_t L, int32_t dim, int32_t k, const rrt_grid* g8,
                          void* scratch, size_t scratch_bytes, void* stream) {
  if (!x1 || !gamma || !beta || !phi || !logits || !wdisp || !rep || !g8 || !scratch || L != g8->L) return RRT_E_INVALID;
  const GridDev gd = to_dev(*g8);
  if (!crmsa_stream4_supported(dim, k, gd) || !crmsa_region4_supported(dim, k, gd))
    return unsupported("crmsa_stream4: dim = 512, k <= 8, regions of 16..576 tokens");
  if (scratch_bytes < 256 + crmsa_region4_scratch_floats(gd, k) * sizeof(float)) return RRT_E_WORKSPACE;
  RRT_TRY(hipMemsetAsync(scratch, 0, 256, (hipStream_t)stream));      // the arrival counters
  return (int)launch_crmsa_stream4(x1, gamma, beta, phi, mean_rstd, logits, wdisp, rep, nullptr, 0,
                                   (float*)((char*)scratch + 256), (int*)scratch, k, gd, (hipStream_t)stream);
}

int rrt_crmsa_dispatch_ln_f32(const float* x1, const float* x0, const float* wdisp,
                              const float* rep2, const float* gamma, const float* beta, float* y, int64_t L,
                              int32_t dim, int32_t k, const rrt_grid* g8, void* stream) {
  if (!x1 || !wdisp || !rep2 || !gamma || !beta || !y || !g8 || L != g8->L) return RRT_E_INVALID;
  if (k <= 0 || k > RRT_MAX_CRMSA_K || dim % 4 || dim > 2048) return unsupported("crmsa: k in [1,8], dim%4==0, dim<=2048");
  return (int)launch_crmsa_dispatch_ln(x1, x0, wdisp, rep2, gamma, beta, y, dim, k, to_dev(*g8),
                                       (hipStream_t)stream);
}

int rrt_crmsa_dispatch_ln_rows_f32(const float* x1, const float* x0, const float* wdisp, const float* rep2, const float* gamma,
                                   const float* beta, float* y, int64_t L, int32_t dim, int32_t k, const rrt_grid* g8, int32_t w,
                                   uint16_t* y16, int32_t prec16, void* stream) {
  if (!x1 || !gamma || !beta || !y || L <= 0 || L > INT32_MAX || dim <= 0 || w < 0 || w > ROWS_W_MAX) return RRT_E_INVALID;
  if (dim % 4 || dim > 2048) return unsupported("dim % 4 == 0, dim <= 2048");
  if (y16 != nullptr && prec16 != RRT_COMPUTE_BF16 && prec16 != RRT_COMPUTE_F16) return RRT_E_INVALID;
  if (k == 0) {      // plain LayerNorm of x1 (+ x0): what rrt_layernorm_f32 runs
    if (wdisp || rep2 || y16) return RRT_E_INVALID;
    return (int)launch_layernorm(x1, x0, gamma, beta, y, (int)L, dim, (hipStream_t)stream, w);
  }
  if (!wdisp || !rep2 || !g8 || L != g8->L) return RRT_E_INVALID;
  if (k < 0 || k > RRT_MAX_CRMSA_K) return unsupported("crmsa: k in [1,8]");
  return (int)launch_crmsa_dispatch_ln(x1, x0, wdisp, rep2, gamma, beta, y, dim, k, to_dev(*g8), (hipStream_t)stream, y16,
                                       y16 ? prec16 : 0, w);
}

int rrt_crmsa_mlp_logits_f32(const float* hid, const float* w2, float* logits, int64_t rows, int32_t hdim,
                             int32_t k, void* stream) {
  if (!hid || !w2 || !logits || rows <= 0 || hdim <= 0) return RRT_E_INVALID;
  if (k <= 0 || k > RRT_MAX_CRMSA_K) return unsupported("crmsa: k in [1,8]");
  return (int)launch_crmsa_mlp_logits(hid, w2, logits, (int)rows, hdim, k, (hipStream_t)stream);
}

int rrt_layernorm_f32(const float* x1, const float* x0, const float* gamma, const float* beta, float* y,
                      int64_t L, int32_t dim, void* stream) {
  if (!x1 || !gamma || !beta || !y || L <= 0 || dim <= 0 || dim % 4) return RRT_E_INVALID;
  if (dim > 2048) return unsupported("dim > 2048");
  return (int)launch_layernorm(x1, x0, gamma, beta, y, (int)L, dim, (hipStream_t)stream);
}

}  // extern "C"

// ------------------------------------------------------------------ row f1: RRTMIL around the encoder
namespace {

// ---- the front every head around the encoder shares: patch_to_emb (Linear + activation in the GEMM epilogue) -> the
// encoder, where the head has one.  rrt_mil_desc / rrt_clam_desc / rrt_dsmil_desc each hold these fields.
// (struct HeadFront: api_internal.h)
HeadFront head_front(const rrt_mil_desc* d) { return HeadFront{&d->enc, d->input_dim, d->emb_act, 1, d->input16}; }
HeadFront head_front(const rrt_clam_desc* d) { return HeadFront{&d->enc, d->input_dim, d->emb_act, d->has_rrt, 0}; }
HeadFront head_front(const rrt_dsmil_desc* d) { return HeadFront{&d->enc, d->input_dim, d->emb_act, d->has_rrt, 0}; }

}  // namespace

// what api_dtfd.hip builds its one-call forward from as well (declared in api_internal.h): the shared front and the ABMIL tail
namespace rrt_api {

// F32X3 concerns the R-MSA layers' big products only (encoder_forward): the GEMMs around the encoder are exact fp32
int gemm_precision(int compute) { return compute == RRT_COMPUTE_F32X3 ? RRT_COMPUTE_F32 : compute; }

int check_head_front(const HeadFront& f, int64_t N) {
  if (N <= 0) return RRT_E_INVALID;
  if (f.has_rrt) {
    int rc = check_desc(f.enc, N);
    if (rc) return rc;
  }
  if (f.input_dim <= 0 || f.input_dim % 32) return unsupported("input_dim must be a positive multiple of 32");
  if (f.emb_act != RRT_ACT_NONE && f.emb_act != RRT_ACT_RELU && f.emb_act != RRT_ACT_GELU)
    return unsupported("emb_act must be none/relu/gelu");
  if (f.enc->compute < 0 || f.enc->compute > RRT_COMPUTE_F32X3) return unsupported("compute must be RRT_COMPUTE_*");
  return RRT_OK;
}

// The workspace of a head's one-call forward: embedding, encoder output, the encoder's own workspace, the head's scratch
// (head_bytes, carved by the head) and the 16-bit images of the reduced-precision modes -- the feature matrix and
// patch_to_emb's weight and, with pool16_hidden > 0, the encoder's output rows and two [pool16_hidden, dim] weights of the
// head's first Linears (0: the head keeps fp32 operands, DSMIL).  The images are part of the size in every mode, so that a
// workspace sized once serves a module that switches modes.
// (struct HeadWs: api_internal.h)
int carve_head(const HeadFront& f, int64_t N, size_t head_bytes, int pool16_hidden, char* base, HeadWs* out) {
  HeadWs w{};
  if (f.has_rrt) {
    int rc = rrt_encoder_workspace_size(f.enc, N, &w.enc_bytes);
    if (rc) return rc;
  }
  const size_t D = f.enc->dim;
  Arena a{base};
  w.emb = a.take((size_t)N * D);
  w.y = a.take((size_t)N * D);
  if (!f.has_rrt) w.y = w.emb;
  w.enc_ws = a.take<char>(w.enc_bytes);
  w.head = a.take<char>(head_bytes);
  w.x16 = a.take<uint16_t>((size_t)N * f.input_dim);
  w.w16 = a.take<uint16_t>(D * f.input_dim);
  if (pool16_hidden > 0) {
    w.y16 = a.take<uint16_t>((size_t)N * D);
    w.pa16 = a.take<uint16_t>((size_t)pool16_hidden * D);
    w.pb16 = a.take<uint16_t>((size_t)pool16_hidden * D);
  }
  w.bytes = a.bytes();
  *out = w;
  return RRT_OK;
}

// patch_to_emb and the encoder of one bag; everything checked by the caller.  pool_a_w / pool_b_w (b may be null): the
// head's first Linears [pool_hidden, dim], whose 16-bit images ride in the one cast launch where the encoder leaves its
// output rows in 16 bits as a by-product (*p16: ws.y16 / pa16 / pb16 are then valid operands); null for a head that keeps
// fp32 operands.  y_out: the caller's buffer for the encoder's output rows instead of ws.y.  tuning: honour the
// RRT_NO_FC16 / RRT_NO_POOL16 tuning variables (RRTMIL).
int head_front_forward(const HeadFront& f, const HeadWs& ws, const float* x, const float* emb_w, const float* emb_b,
                       const rrt_encoder_weights* enc_w, const float* pool_a_w, const float* pool_b_w, int pool_hidden,
                       float* y_out, bool tuning, int64_t N, void* stream, bool* p16) {
  static const bool env_no_fc16 = rrt_tune_env("RRT_NO_FC16") != nullptr;
  static const bool env_no_pool16 = rrt_tune_env("RRT_NO_POOL16") != nullptr;
  const int D = f.enc->dim;
  hipStream_t st = (hipStream_t)stream;
  const int gemm_prec = gemm_precision(f.enc->compute);
  LinearEpilogue ep{};
  ep.prec = gemm_prec;
  ep.bias = emb_b;
  ep.act = f.emb_act;
  // Reduced-precision modes (round 5): the features and the weight are cast to 16 bits by one streaming launch and the GEMM
  // runs on 16-bit operands through LDS-DMA.  The fp32-operand kernel rounds the same values to the same 16-bit numbers,
  // but after staging them in LDS as fp32: twice the DMA bytes through a path that is issue-bound (41 us at
  // N = 9000 x 1024 against ~10 + ~13 here).
  const bool fc16 = !(tuning && env_no_fc16) && (gemm_prec == RRT_COMPUTE_BF16 || gemm_prec == RRT_COMPUTE_F16) &&
                    f.input_dim % 64 == 0;
  if (f.input16 != 0 && (f.input16 != gemm_prec || !fc16))
    return unsupported("rrt_mil_forward: 16-bit features (input16) need enc.compute == input16 (bf16 / f16) and input_dim % 64 == 0");
  bool pool16 = false, y16_done = false;
  if (fc16) {
    const uint16_t* x16 = ws.x16;
    Cast16Jobs cj{};
    if (f.input16) {                 // the caller's features ARE the 16-bit operand: only the weight is cast
      x16 = (const uint16_t*)x;
    } else {
      cj.add(x, ws.x16, (size_t)N * f.input_dim);
    }
    cj.add(emb_w, ws.w16, (size_t)D * f.input_dim);
    // the head's first Linears' weights in the same launch (their 16-bit-operand product reads the encoder's y16)
    pool16 = pool_a_w && ws.y16 && !(tuning && env_no_pool16) && f.has_rrt && D % 64 == 0 &&
             ((size_t)pool_hidden * D) % 4 == 0 && cj.count + 2 <= CAST16_MAX_JOBS;
    if (pool16) {
      cj.add(pool_a_w, ws.pa16, (size_t)pool_hidden * D);
      if (pool_b_w) cj.add(pool_b_w, ws.pb16, (size_t)pool_hidden * D);
    }
    RRT_TRY(launch_cast16(cj, gemm_prec, st));
    RRT_TRY(launch_linear16(x16, ws.w16, ws.emb, (int)N, D, f.input_dim, ep, st));
  } else {
    RRT_TRY(launch_linear(x, emb_w, ws.emb, (int)N, D, f.input_dim, ep, st));
  }
  if (f.has_rrt) {
    int rc = encoder_forward(f.enc, enc_w, ws.emb, y_out ? y_out : ws.y, N, ws.enc_ws, ws.enc_bytes, stream, nullptr, nullptr,
                             nullptr, pool16 ? ws.y16 : nullptr, &y16_done);
    if (rc) return rc;
  }
  *p16 = pool16 && y16_done;
  return RRT_OK;
}

// (struct PoolWs: api_internal.h)
PoolWs carve_pool(int64_t N, int dim, int hidden, int gated, char* base) {
  PoolWs w{};
  Arena a{base};
  const size_t nb = (size_t)(N + POOL_CHUNK - 1) / POOL_CHUNK;
  w.hid_a = a.take((size_t)N * hidden);
  if (gated) w.hid_b = a.take((size_t)N * hidden);
  w.a_raw = a.take((size_t)N);
  w.part = a.take(nb * ((size_t)dim + 4));
  w.bytes = a.bytes();
  return w;
}

int check_pool(int64_t N, int dim, int hidden, int act, int n_classes) {
  if (N <= 0 || dim <= 0 || hidden <= 0 || n_classes <= 0) return RRT_E_INVALID;
  if (dim % 32) return unsupported("pool: dim must be a multiple of 32");
  if (hidden % 4) return unsupported("pool: hidden width must be a multiple of 4");
  if (act < RRT_ACT_NONE || act > RRT_ACT_TANH) return unsupported("pool: act must be none/relu/gelu/tanh");
  if (N > (int64_t)1000000) return unsupported("pool: bag larger than 1e6 tokens");
  if (!pool_merge_fits(N, dim)) return unsupported("pool: the merge block's LDS (4 * (n_tokens / 32 + dim) + 16 KB) is above 150 KB");
  return RRT_OK;
}
// the pooling alone (rrt_attn_pool_*): one workspace query serves the forward and the backward, so all three refuse what
// either launch cannot hold
int check_attn_pool(int64_t N, int dim, int hidden) {
  int rc = check_pool(N, dim, hidden, RRT_ACT_NONE, 1);
  if (rc) return rc;
  if (!pool_backward_fits(dim, hidden))
    return unsupported("attn pool: the backward block's LDS (4 * (dim + 4 * (hidden + 4))) is above 64 KB");
  return RRT_OK;
}

int pool_predict(const float* y, const float* a_w, const float* a_b, const float* b_w, const float* b_b,
                 const float* c_w, const float* c_b, const float* pred_w, const float* pred_b, float* pooled,
                 float* logits, float* attn, int no_norm, int64_t N, int dim, int hidden, int act,
                 int n_classes, int compute, const PoolWs& ws, hipStream_t st, const uint16_t* y16, const uint16_t* a_w16,
                 const uint16_t* b_w16) {
  LinearEpilogue ep{};
  ep.prec = compute;
  ep.bias = a_b;
  ep.act = act;
  // (round 5: the 16-bit-operand route as patch_to_emb's -- rows cast once by a launch of their own, GEMM on 16-bit images --
  // was measured here and lost: configs[2] 10.55-10.60 k against 10.71-10.80 k slides/s; the cast's 28 MB cost more than the
  // narrow GEMM saved.  Round 6: the encoder's last kernel leaves the rows in 16 bits as a by-product (y16: 9 MB more written,
  // no launch, no second read of y) and the weights ride in the classifier's one cast launch: the fp32-operand product --
  // 23 us for 1.2 GFLOP: 142 blocks on 256 CUs, twice the bytes through the LDS-DMA path -- becomes a 16-bit-operand one)
  const bool p16 = y16 != nullptr && a_w16 != nullptr && (!b_w || b_w16 != nullptr) && dim % 64 == 0 &&
                   (compute == RRT_COMPUTE_BF16 || compute == RRT_COMPUTE_F16);
  RRT_TRY(p16 ? launch_linear16(y16, a_w16, ws.hid_a, (int)N, hidden, dim, ep, st)
              : launch_linear(y, a_w, ws.hid_a, (int)N, hidden, dim, ep, st));
  if (b_w) {
    ep.bias = b_b;
    ep.act = RRT_ACT_SIGMOID;
    RRT_TRY(p16 ? launch_linear16(y16, b_w16, ws.hid_b, (int)N, hidden, dim, ep, st)
                : launch_linear(y, b_w, ws.hid_b, (int)N, hidden, dim, ep, st));
  }
  RRT_TRY(launch_pool_partial(y, ws.hid_a, b_w ? ws.hid_b : nullptr, c_w, c_b, ws.a_raw, ws.part, (int)N, dim, hidden, st));
  return (int)launch_pool_merge(ws.part, ws.a_raw, pred_w, pred_b, pooled, logits, attn, no_norm, (int)N, dim, n_classes, st);
}

}  // namespace rrt_api

namespace {

int check_mil(const rrt_mil_desc* d, int64_t N) {
  if (!d) return RRT_E_INVALID;
  int rc = check_head_front(head_front(d), N);
  if (rc) return rc;
  return check_pool(N, d->enc.dim, d->pool_hidden, d->pool_act, d->n_classes);
}

// RRTMIL's workspace: the shared head layout around carve_pool's scratch
int carve_mil(const rrt_mil_desc* d, int64_t N, char* base, HeadWs* hw, PoolWs* pws) {
  int rc = carve_head(head_front(d), N, carve_pool(N, d->enc.dim, d->pool_hidden, d->pool_gated, nullptr).bytes, d->pool_hidden,
                      base, hw);
  if (rc == RRT_OK && pws) *pws = carve_pool(N, d->enc.dim, d->pool_hidden, d->pool_gated, hw->head);
  return rc;
}

// ---- CLAM heads (clam_pool.hip)
int check_branch_pool(int64_t N, int dim, int hidden, int K) {
  if (N <= 0 || dim <= 0 || hidden <= 0) return RRT_E_INVALID;
  if (K < 1 || K > 8) return unsupported("branch pool: 1 <= n_branches <= 8");
  if (dim % 32) return unsupported("branch pool: dim must be a multiple of 32");
  if (dim > 2048) return unsupported("branch pool: dim > 2048");
  if (hidden % 4) return unsupported("branch pool: hidden width must be a multiple of 4");
  if (N > (int64_t)1000000) return unsupported("branch pool: bag larger than 1e6 tokens");
  return RRT_OK;
}

size_t branch_pool_workspace(int64_t N, int dim, int hidden, int K) {
  const size_t fwd = align_up(branch_pool_part_floats((int)N, dim, K) * sizeof(float), 256);
  const size_t bwd = align_up(branch_pool_backward_part_floats((int)N, hidden, K) * sizeof(float), 256);
  return fwd > bwd ? fwd : bwd;
}

struct ClamWs {
  float *hid_a, *hid_b, *a_raw, *attn, *pooled, *part;
  size_t bytes;
};
ClamWs carve_clam(int64_t N, int dim, int hidden, int gated, int K, char* base) {
  ClamWs w{};
  Arena a{base};
  w.hid_a = a.take((size_t)N * hidden);
  if (gated) w.hid_b = a.take((size_t)N * hidden);
  w.a_raw = a.take((size_t)K * N);
  w.attn = a.take((size_t)K * N);
  w.pooled = a.take((size_t)K * dim);
  w.part = a.take(branch_pool_part_floats((int)N, dim, K));
  w.bytes = a.bytes();
  return w;
}

int check_clam(const rrt_clam_desc* d, int64_t N) {
  if (!d) return RRT_E_INVALID;
  int rc = check_head_front(head_front(d), N);
  if (rc) return rc;
  if (d->n_classes <= 0) return RRT_E_INVALID;
  if (d->per_branch && d->n_classes > 8) return unsupported("CLAM_MB: n_classes <= 8 (one attention branch per class)");
  return check_branch_pool(N, d->enc.dim, d->hidden, d->per_branch ? d->n_classes : 1);
}

// the CLAM heads' workspace: the shared head layout around carve_clam's scratch
int carve_clam_head(const rrt_clam_desc* d, int64_t N, char* base, HeadWs* hw, ClamWs* cws) {
  const int K = d->per_branch ? d->n_classes : 1;
  int rc = carve_head(head_front(d), N, carve_clam(N, d->enc.dim, d->hidden, d->gated, K, nullptr).bytes, d->hidden, base, hw);
  if (rc == RRT_OK && cws) *cws = carve_clam(N, d->enc.dim, d->hidden, d->gated, K, hw->head);
  return rc;
}

// ---- DSMIL head (dsmil_pool.hip)
int check_instance_max(int64_t N, int dim, int C) {
  if (N <= 0 || dim <= 0) return RRT_E_INVALID;
  if (C < 1 || C > 8) return unsupported("instance max: 1 <= n_classes <= 8");
  if (dim % 32) return unsupported("instance max: dim must be a multiple of 32");
  if (dim > 2048) return unsupported("instance max: dim > 2048");
  if (N > (int64_t)1000000) return unsupported("instance max: bag larger than 1e6 tokens");
  return RRT_OK;
}

struct IMaxWs {
  float* pv;
  int* pi;
  size_t bytes;
};
IMaxWs carve_imax(int64_t N, int C, char* base) {
  IMaxWs w{};
  Arena a{base};
  const size_t rec = (size_t)instance_max_part_records((int)N) * C;
  w.pv = a.take(rec);
  w.pi = a.take<int>(rec);
  w.bytes = a.bytes();
  return w;
}

int check_dsmil_pool(int64_t N, int dim, int Q, int C) {
  if (N <= 0 || dim <= 0 || Q <= 0) return RRT_E_INVALID;
  if (C < 1 || C > 8) return unsupported("dsmil pool: 1 <= n_classes <= 8");
  if (dim % 32) return unsupported("dsmil pool: dim must be a multiple of 32");
  if (dim > 2048) return unsupported("dsmil pool: dim > 2048");
  if (Q % 4) return unsupported("dsmil pool: q_dim must be a multiple of 4");
  if (Q > 4096) return unsupported("dsmil pool: q_dim > 4096");
  if (N > (int64_t)1000000) return unsupported("dsmil pool: bag larger than 1e6 tokens");
  return RRT_OK;
}

struct DsmilWs {
  float *v, *vb, *raw, *lpart, *part;
  size_t bytes;
};
DsmilWs carve_dsmil_pool(int64_t N, int dim, int C, char* base) {
  DsmilWs w{};
  Arena a{base};
  w.v = a.take((size_t)C * dim);
  w.vb = a.take(16);
  w.lpart = a.take(64);
  w.raw = a.take((size_t)N * C);
  w.part = a.take(dsmil_pool_part_floats((int)N, dim, C));
  w.bytes = a.bytes();
  return w;
}

int check_dsmil(const rrt_dsmil_desc* d, int64_t N) {
  if (!d) return RRT_E_INVALID;
  int rc = check_head_front(head_front(d), N);
  if (rc) return rc;
  rc = check_instance_max(N, d->enc.dim, d->n_classes);
  if (rc) return rc;
  return check_dsmil_pool(N, d->enc.dim, d->q_dim, d->n_classes);
}

// MILNet's workspace: the shared head layout (no 16-bit images behind the encoder) around the two streams' scratch and one
// 256-byte piece for the critical instances [8] and the class maxima [8] of a caller that does not ask for them
struct DsmilHeadWs {
  IMaxWs imax;
  DsmilWs pool;
  long long* argmax;
  float* cmax;
  size_t bytes;
};
DsmilHeadWs carve_dsmil_scratch(int64_t N, int dim, int C, char* base) {
  DsmilHeadWs w{};
  Arena a{base};
  w.imax = carve_imax(N, C, a.take<char>(carve_imax(N, C, nullptr).bytes));
  w.pool = carve_dsmil_pool(N, dim, C, a.take<char>(carve_dsmil_pool(N, dim, C, nullptr).bytes));
  char* tail = a.take<char>(256);
  w.argmax = (long long*)tail;
  w.cmax = tail ? (float*)(tail + 64) : nullptr;
  w.bytes = a.bytes();
  return w;
}
int carve_dsmil_head(const rrt_dsmil_desc* d, int64_t N, char* base, HeadWs* hw, DsmilHeadWs* dws) {
  int rc = carve_head(head_front(d), N, carve_dsmil_scratch(N, d->enc.dim, d->n_classes, nullptr).bytes, 0, base, hw);
  if (rc == RRT_OK && dws) *dws = carve_dsmil_scratch(N, d->enc.dim, d->n_classes, hw->head);
  return rc;
}

// ---- ABMIL / gated ABMIL / IBMIL / MeanMIL / MaxMIL heads (bag_pool.hip + the pools above)
HeadFront head_front(const rrt_bagmil_desc* d) { return HeadFront{&d->enc, d->input_dim, d->emb_act, d->has_rrt, 0}; }

int check_bag_mean(int64_t N, int dim, int C) {
  if (N <= 0 || dim <= 0) return RRT_E_INVALID;
  if (C < 1 || C > 8) return unsupported("bag mean: 1 <= n_classes <= 8");
  if (dim % 32) return unsupported("bag mean: dim must be a multiple of 32");
  if (dim > 2048) return unsupported("bag mean: dim > 2048");
  if (N > (int64_t)1000000) return unsupported("bag mean: bag larger than 1e6 tokens");
  return RRT_OK;
}

struct MeanWs {
  float *part1, *part2;
  size_t bytes;
};
MeanWs carve_mean(int64_t N, int dim, char* base) {
  MeanWs w{};
  Arena a{base};
  w.part1 = a.take(bag_mean_part1_rows((int)N) * dim);
  w.part2 = a.take(bag_mean_part2_rows((int)N) * dim);
  w.bytes = a.bytes();
  return w;
}

int check_deconf(int dim, int K, int V, int J, int C) {
  if (dim <= 0 || V <= 0 || J <= 0 || C <= 0) return RRT_E_INVALID;
  if (K < 1 || K > 64) return unsupported("deconfounder: 1 <= n_conf <= 64");
  if (dim % 32 || dim > 2048) return unsupported("deconfounder: dim must be a multiple of 32 up to 2048");
  if (V % 32 || V > 2048) return unsupported("deconfounder: conf_dim must be a multiple of 32 up to 2048");
  if (J % 4 || J > 512) return unsupported("deconfounder: joint_dim must be a multiple of 4 up to 512");
  return RRT_OK;
}

bool bagmil_attn(int pool) { return pool == RRT_BAGPOOL_ATTN || pool == RRT_BAGPOOL_ATTN_GATED || pool == RRT_BAGPOOL_ATTN_DECONF; }
int bagmil_pool_act(const rrt_bagmil_desc* d) { return d->pool == RRT_BAGPOOL_ATTN_GATED ? d->pool_act : RRT_ACT_TANH; }

int check_bagmil(const rrt_bagmil_desc* d, int64_t N) {
  if (!d) return RRT_E_INVALID;
  int rc = check_head_front(head_front(d), N);
  if (rc) return rc;
  if (d->n_classes <= 0) return RRT_E_INVALID;
  switch (d->pool) {
    case RRT_BAGPOOL_MEAN: return check_bag_mean(N, d->enc.dim, d->n_classes);
    case RRT_BAGPOOL_MAX: return check_instance_max(N, d->enc.dim, d->n_classes);
    case RRT_BAGPOOL_ATTN:
    case RRT_BAGPOOL_ATTN_GATED:
    case RRT_BAGPOOL_ATTN_DECONF:
      rc = check_pool(N, d->enc.dim, d->pool_hidden, bagmil_pool_act(d), d->n_classes);
      if (rc) return rc;
      if (d->enc.dim > 2048) return unsupported("pool: dim > 2048");
      if (d->pool == RRT_BAGPOOL_ATTN_DECONF) return check_deconf(d->enc.dim, d->deconf_k, d->deconf_v, d->deconf_j, d->n_classes);
      return RRT_OK;
    default: return unsupported("pool must be RRT_BAGPOOL_*");
  }
}

// the tail's scratch: ONE carve for whichever pool the head has, plus a 256-byte piece for the critical instances of a MAX
// caller that does not ask for them and a [dim] row for the deconfounder's input when the caller does not ask for `pooled`
struct BagmilWs {
  PoolWs pool;
  IMaxWs imax;
  MeanWs mean;
  long long* argmax;
  float* pooled;
  size_t bytes;
};
BagmilWs carve_bagmil_scratch(const rrt_bagmil_desc* d, int64_t N, char* base) {
  BagmilWs w{};
  Arena a{base};
  const int D = d->enc.dim;
  if (d->pool == RRT_BAGPOOL_MEAN) {
    w.mean = carve_mean(N, D, a.take<char>(carve_mean(N, D, nullptr).bytes));
  } else if (d->pool == RRT_BAGPOOL_MAX) {
    w.imax = carve_imax(N, d->n_classes, a.take<char>(carve_imax(N, d->n_classes, nullptr).bytes));
    w.argmax = (long long*)a.take<char>(256);
  } else {
    const int gated = d->pool == RRT_BAGPOOL_ATTN_GATED;
    w.pool = carve_pool(N, D, d->pool_hidden, gated, a.take<char>(carve_pool(N, D, d->pool_hidden, gated, nullptr).bytes));
    w.pooled = a.take((size_t)D);
  }
  w.bytes = a.bytes();
  return w;
}
int carve_bagmil_head(const rrt_bagmil_desc* d, int64_t N, char* base, HeadWs* hw, BagmilWs* bws) {
  int rc = carve_head(head_front(d), N, carve_bagmil_scratch(d, N, nullptr).bytes, bagmil_attn(d->pool) ? d->pool_hidden : 0, base,
                      hw);
  if (rc == RRT_OK && bws) *bws = carve_bagmil_scratch(d, N, hw->head);
  return rc;
}

}  // namespace

extern "C" {

int rrt_linear_act_f32(const float* A, const float* B, const float* bias, float* C, int64_t M, int32_t N,
                       int32_t K, int32_t act, int32_t compute, void* stream) {
  if (!A || !B || !C || M <= 0 || N <= 0 || K <= 0) return RRT_E_INVALID;
  if (K % 32) return unsupported("linear: K must be a multiple of 32");
  if (compute < 0 || compute > 2) return unsupported("compute must be RRT_COMPUTE_F32/BF16/F16");
  if (act < RRT_ACT_NONE || act > RRT_ACT_SIGMOID) return unsupported("unknown activation");
  LinearEpilogue ep{};
  ep.prec = compute;
  ep.bias = bias;
  ep.act = act;
  return (int)launch_linear(A, B, C, (int)M, N, K, ep, (hipStream_t)stream);
}

int rrt_pool_workspace_size(int64_t n_tokens, int32_t dim, int32_t hidden, int32_t gated, size_t* bytes) {
  if (!bytes) return RRT_E_INVALID;
  int rc = check_pool(n_tokens, dim, hidden, RRT_ACT_NONE, 1);
  if (rc) return rc;
  *bytes = carve_pool(n_tokens, dim, hidden, gated, nullptr).bytes;
  return RRT_OK;
}

int rrt_pool_predict_f32(const float* y, const float* a_w, const float* a_b, const float* b_w, const float* b_b,
                         const float* c_w, const float* c_b, const float* pred_w, const float* pred_b,
                         float* pooled, float* logits, float* attn, int32_t no_norm, int64_t n_tokens,
                         int32_t dim, int32_t hidden, int32_t act, int32_t n_classes, int32_t compute,
                         void* workspace, size_t workspace_bytes, void* stream) {
  if (!y || !a_w || !c_w || !pred_w || !logits) return RRT_E_INVALID;
  int rc = check_pool(n_tokens, dim, hidden, act, n_classes);
  if (rc) return rc;
  if (compute < 0 || compute > 2) return unsupported("compute must be RRT_COMPUTE_F32/BF16/F16");
  const int gated = b_w != nullptr;
  if (!workspace || workspace_bytes < carve_pool(n_tokens, dim, hidden, gated, nullptr).bytes) return RRT_E_WORKSPACE;
  PoolWs ws = carve_pool(n_tokens, dim, hidden, gated, (char*)workspace);
  return pool_predict(y, a_w, a_b, b_w, b_b, c_w, c_b, pred_w, pred_b, pooled, logits, attn, no_norm, n_tokens,
                      dim, hidden, act, n_classes, compute, ws, (hipStream_t)stream);
}

// ---- the pooling alone, forward and backward (training: the first Linear + activation stay autograd-visible layers)
int rrt_attn_pool_workspace_size(int64_t n_tokens, int32_t dim, int32_t hidden, size_t* bytes) {
  if (!bytes) return RRT_E_INVALID;
  int rc = check_attn_pool(n_tokens, dim, hidden);
  if (rc) return rc;
  const size_t nb = (size_t)(n_tokens + POOL_CHUNK - 1) / POOL_CHUNK;
  const size_t fwd = align_up(nb * ((size_t)dim + 4) * sizeof(float), 256);
  const size_t bwd = align_up(pool_backward_part_floats((int)n_tokens, hidden) * sizeof(float), 256);
  *bytes = fwd > bwd ? fwd : bwd;
  return RRT_OK;
}

int rrt_attn_pool_f32(const float* y, const float* hid_a, const float* hid_b, const float* c_w, const float* c_b,
                      float* pooled, float* attn, float* a_raw, int64_t n_tokens, int32_t dim, int32_t hidden,
                      void* workspace, size_t workspace_bytes, void* stream) {
  if (!y || !hid_a || !c_w || !pooled || !attn || !a_raw) return RRT_E_INVALID;
  int rc = check_attn_pool(n_tokens, dim, hidden);
  if (rc) return rc;
  size_t need = 0;
  (void)rrt_attn_pool_workspace_size(n_tokens, dim, hidden, &need);
  if (!workspace || workspace_bytes < need) return RRT_E_WORKSPACE;
  RRT_TRY(launch_pool_partial(y, hid_a, hid_b, c_w, c_b, a_raw, (float*)workspace, (int)n_tokens, dim, hidden, (hipStream_t)stream));
  return (int)launch_pool_merge((const float*)workspace, a_raw, nullptr, nullptr, pooled, nullptr, attn, 0, (int)n_tokens, dim, 0,
                                (hipStream_t)stream);
}

int rrt_attn_pool_backward_f32(const float* y, const float* hid_a, const float* hid_b, const float* c_w, const float* attn,
                               const float* pooled, const float* d_pooled, const float* d_attn, const float* d_raw,
                               const float* c_ext, float* dy, float* dhid_a, float* dhid_b, float* dwcb, int64_t n_tokens,
                               int32_t dim, int32_t hidden, void* workspace, size_t workspace_bytes, void* stream) {
  if (!y || !hid_a || !c_w || !attn || !pooled || !d_pooled || !dy || !dhid_a || !dwcb || (hid_b && !dhid_b)) return RRT_E_INVALID;
  int rc = check_attn_pool(n_tokens, dim, hidden);
  if (rc) return rc;
  if (d_attn && !c_ext) return RRT_E_INVALID;     // c_ext = sum_n attn_n d_attn_n (device scalar) goes with d_attn
  size_t need = 0;
  (void)rrt_attn_pool_workspace_size(n_tokens, dim, hidden, &need);
  if (!workspace || workspace_bytes < need) return RRT_E_WORKSPACE;
  return (int)launch_pool_backward(y, hid_a, hid_b, c_w, attn, pooled, d_pooled, d_attn, d_raw, c_ext, dy, dhid_a, dhid_b, dwcb,
                                   (float*)workspace, (int)n_tokens, dim, hidden, (hipStream_t)stream);
}

int rrt_mil_workspace_size(const rrt_mil_desc* desc, int64_t n_tokens, size_t* bytes) {
  if (!bytes) return RRT_E_INVALID;
  int rc = check_mil(desc, n_tokens);
  if (rc) return rc;
  HeadWs hw;
  rc = carve_mil(desc, n_tokens, nullptr, &hw, nullptr);
  if (rc) return rc;
  *bytes = hw.bytes;
  return RRT_OK;
}

int rrt_mil_forward_f32(const rrt_mil_desc* desc, const rrt_mil_weights* w, const float* x, float* logits,
                        float* attn, int32_t no_norm, float* feat, int64_t n_tokens, void* workspace,
                        size_t workspace_bytes, void* stream) {
  if (!desc || !w || !x || !logits) return RRT_E_INVALID;
  int rc = check_mil(desc, n_tokens);
  if (rc) return rc;
  if (!w->emb_w || !w->pool_a_w || !w->pool_c_w || !w->pred_w || (desc->pool_gated && !w->pool_b_w))
    return RRT_E_INVALID;
  HeadWs hw;
  PoolWs pws;
  rc = carve_mil(desc, n_tokens, (char*)workspace, &hw, &pws);
  if (rc) return rc;
  if (!workspace || workspace_bytes < hw.bytes) return RRT_E_WORKSPACE;
  const float* pool_b_w = desc->pool_gated ? w->pool_b_w : nullptr;
  float* y = feat ? feat : hw.y;
  bool p16 = false;
  rc = head_front_forward(head_front(desc), hw, x, w->emb_w, w->emb_b, &w->enc, w->pool_a_w, pool_b_w, desc->pool_hidden, y,
                          /*tuning=*/true, n_tokens, stream, &p16);
  if (rc) return rc;
  return pool_predict(y, w->pool_a_w, w->pool_a_b, pool_b_w, w->pool_b_b, w->pool_c_w, w->pool_c_b, w->pred_w, w->pred_b,
                      nullptr, logits, attn, no_norm, n_tokens, desc->enc.dim, desc->pool_hidden, desc->pool_act,
                      desc->n_classes, gemm_precision(desc->enc.compute), pws, (hipStream_t)stream, p16 ? hw.y16 : nullptr,
                      p16 ? hw.pa16 : nullptr, (p16 && pool_b_w) ? hw.pb16 : nullptr);
}

// ---- CLAM heads: the branch pool alone (forward, backward), top-k of rows, and the one-call CLAM_SB / CLAM_MB forward
int rrt_branch_pool_workspace_size(int64_t n_tokens, int32_t dim, int32_t hidden, int32_t n_branches, size_t* bytes) {
  if (!bytes) return RRT_E_INVALID;
  int rc = check_branch_pool(n_tokens, dim, hidden, n_branches);
  if (rc) return rc;
  *bytes = branch_pool_workspace(n_tokens, dim, hidden, n_branches);
  return RRT_OK;
}

int rrt_branch_pool_f32(const float* y, const float* hid_a, const float* hid_b, const float* c_w, const float* c_b,
                        float* pooled, float* attn, float* a_raw, int64_t n_tokens, int32_t dim, int32_t hidden,
                        int32_t n_branches, void* workspace, size_t workspace_bytes, void* stream) {
  if (!y || !hid_a || !c_w || !pooled || !a_raw) return RRT_E_INVALID;
  int rc = check_branch_pool(n_tokens, dim, hidden, n_branches);
  if (rc) return rc;
  if (!pool_merge_fits(n_tokens, dim)) return unsupported("branch pool: bag too large for the merge block");
  if (!workspace || workspace_bytes < branch_pool_workspace(n_tokens, dim, hidden, n_branches)) return RRT_E_WORKSPACE;
  return (int)launch_branch_pool(y, hid_a, hid_b, c_w, c_b, nullptr, nullptr, pooled, nullptr, attn, a_raw, (float*)workspace, 0,
                                 0, (int)n_tokens, dim, hidden, n_branches, (hipStream_t)stream);
}

int rrt_branch_pool_backward_f32(const float* y, const float* hid_a, const float* hid_b, const float* c_w, const float* attn,
                                 const float* pooled, const float* d_pooled, const float* d_raw, float* dy, float* dhid_a,
                                 float* dhid_b, float* dwcb, int64_t n_tokens, int32_t dim, int32_t hidden, int32_t n_branches,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  if (!y || !hid_a || !c_w || !attn || !pooled || !d_pooled || !dy || !dhid_a || !dwcb || (hid_b && !dhid_b)) return RRT_E_INVALID;
  int rc = check_branch_pool(n_tokens, dim, hidden, n_branches);
  if (rc) return rc;
  if (branch_pool_backward_lds(dim, hidden, n_branches) > POOL_MERGE_LDS_MAX)
    return unsupported("branch pool backward: n_branches * (dim + 4 * hidden) floats exceed the block's LDS budget");
  if (!workspace || workspace_bytes < branch_pool_workspace(n_tokens, dim, hidden, n_branches)) return RRT_E_WORKSPACE;
  return (int)launch_branch_pool_backward(y, hid_a, hid_b, c_w, attn, pooled, d_pooled, d_raw, dy, dhid_a, dhid_b, dwcb,
                                          (float*)workspace, (int)n_tokens, dim, hidden, n_branches, (hipStream_t)stream);
}

int rrt_topk_rows_f32(const float* x, int64_t* idx, int32_t n_rows, int64_t n, int32_t k, void* stream) {
  if (!x || !idx || n_rows <= 0 || n <= 0 || k <= 0) return RRT_E_INVALID;
  if (k > 32) return unsupported("topk: k <= 32");
  if (n > (int64_t)2147483646) return unsupported("topk: rows of at most 2^31 - 2 values");
  if (n_rows > 65535) return unsupported("topk: at most 65535 rows");
  if (n < k) return RRT_E_INVALID;
  return (int)launch_topk_rows(x, (long long*)idx, n_rows, (int)n, k, (hipStream_t)stream);
}

int rrt_clam_workspace_size(const rrt_clam_desc* desc, int64_t n_tokens, size_t* bytes) {
  if (!bytes) return RRT_E_INVALID;
  int rc = check_clam(desc, n_tokens);
  if (rc) return rc;
  HeadWs hw;
  rc = carve_clam_head(desc, n_tokens, nullptr, &hw, nullptr);
  if (rc) return rc;
  *bytes = hw.bytes;
  return RRT_OK;
}

int rrt_clam_forward_f32(const rrt_clam_desc* desc, const rrt_clam_weights* w, const float* x, float* logits, float* a_raw,
                         float* attn, float* features, int64_t* topk_idx, int64_t n_tokens, void* workspace,
                         size_t workspace_bytes, void* stream) {
  if (!desc || !w || !x || !logits) return RRT_E_INVALID;
  int rc = check_clam(desc, n_tokens);
  if (rc) return rc;
  if (!w->emb_w || !w->a_w || !w->c_w || !w->cls_w || (desc->gated && !w->b_w)) return RRT_E_INVALID;
  if (topk_idx) {
    if (desc->k_sample <= 0) return RRT_E_INVALID;
    if (desc->k_sample > 32) return unsupported("topk: k <= 32");
    if (n_tokens < desc->k_sample) return RRT_E_INVALID;
  }
  if (!pool_merge_fits(n_tokens, desc->enc.dim)) return unsupported("branch pool: bag too large for the merge block");
  HeadWs hw;
  ClamWs cws;
  rc = carve_clam_head(desc, n_tokens, (char*)workspace, &hw, &cws);
  if (rc) return rc;
  if (!workspace || workspace_bytes < hw.bytes) return RRT_E_WORKSPACE;
  const int D = desc->enc.dim, K = desc->per_branch ? desc->n_classes : 1, H = desc->hidden;
  hipStream_t st = (hipStream_t)stream;
  const float* y = hw.y;
  bool p16 = false;
  rc = head_front_forward(head_front(desc), hw, x, w->emb_w, w->emb_b, &w->enc, w->a_w, desc->gated ? w->b_w : nullptr, H,
                          nullptr, /*tuning=*/false, n_tokens, stream, &p16);
  if (rc) return rc;
  // the gate Linears: on the encoder's 16-bit rows and the weight images of the front's cast launch where it left them
  LinearEpilogue ep{};
  ep.prec = gemm_precision(desc->enc.compute);
  ep.bias = w->a_b;
  ep.act = RRT_ACT_TANH;
  RRT_TRY(p16 ? launch_linear16(hw.y16, hw.pa16, cws.hid_a, (int)n_tokens, H, D, ep, st)
              : launch_linear(y, w->a_w, cws.hid_a, (int)n_tokens, H, D, ep, st));
  if (desc->gated) {
    ep.bias = w->b_b;
    ep.act = RRT_ACT_SIGMOID;
    RRT_TRY(p16 ? launch_linear16(hw.y16, hw.pb16, cws.hid_b, (int)n_tokens, H, D, ep, st)
                : launch_linear(y, w->b_w, cws.hid_b, (int)n_tokens, H, D, ep, st));
  }
  float* raw = a_raw ? a_raw : cws.a_raw;
  float* at = attn ? attn : (topk_idx ? cws.attn : nullptr);
  RRT_TRY(launch_branch_pool(y, cws.hid_a, desc->gated ? cws.hid_b : nullptr, w->c_w, w->c_b, w->cls_w, w->cls_b,
                             features ? features : cws.pooled, logits, at, raw, cws.part, desc->per_branch, desc->n_classes,
                             (int)n_tokens, D, H, K, st));
  if (topk_idx) RRT_TRY(launch_topk_rows(at, (long long*)topk_idx, K, (int)n_tokens, desc->k_sample, st));
  return RRT_OK;
}

// ---- DSMIL head: the instance stream and the bag stream alone, and the one-call MILNet forward
int rrt_instance_max_workspace_size(int64_t n_tokens, int32_t dim, int32_t n_classes, size_t* bytes) {
  if (!bytes) return RRT_E_INVALID;
  int rc = check_instance_max(n_tokens, dim, n_classes);
  if (rc) return rc;
  *bytes = carve_imax(n_tokens, n_classes, nullptr).bytes;
  return RRT_OK;
}

int rrt_instance_max_f32(const float* y, const float* w, const float* b, float* classes, float* cmax, int64_t* argmax,
                         int64_t n_tokens, int32_t dim, int32_t n_classes, void* workspace, size_t workspace_bytes,
                         void* stream) {
  if (!y || !w || !argmax) return RRT_E_INVALID;
  int rc = check_instance_max(n_tokens, dim, n_classes);
  if (rc) return rc;
  if (!workspace || workspace_bytes < carve_imax(n_tokens, n_classes, nullptr).bytes) return RRT_E_WORKSPACE;
  IMaxWs ws = carve_imax(n_tokens, n_classes, (char*)workspace);
  return (int)launch_instance_max(y, w, b, classes, cmax, (long long*)argmax, ws.pv, ws.pi, (int)n_tokens, dim, n_classes,
                                  (hipStream_t)stream);
}

int rrt_dsmil_pool_workspace_size(int64_t n_tokens, int32_t dim, int32_t q_dim, int32_t n_classes, size_t* bytes) {
  if (!bytes) return RRT_E_INVALID;
  int rc = check_dsmil_pool(n_tokens, dim, q_dim, n_classes);
  if (rc) return rc;
  *bytes = carve_dsmil_pool(n_tokens, dim, n_classes, nullptr).bytes;
  return RRT_OK;
}

int rrt_dsmil_pool_f32(const float* feats, const int64_t* argmax, const float* q_w, const float* q_b, const float* fcc_w,
                       const float* fcc_b, float* logits, float* A, float* B, float* a_raw, int64_t n_tokens, int32_t dim,
                       int32_t q_dim, int32_t n_classes, void* workspace, size_t workspace_bytes, void* stream) {
  if (!feats || !argmax || !q_w || !fcc_w || !logits) return RRT_E_INVALID;
  int rc = check_dsmil_pool(n_tokens, dim, q_dim, n_classes);
  if (rc) return rc;
  if (!workspace || workspace_bytes < carve_dsmil_pool(n_tokens, dim, n_classes, nullptr).bytes) return RRT_E_WORKSPACE;
  DsmilWs ws = carve_dsmil_pool(n_tokens, dim, n_classes, (char*)workspace);
  return (int)launch_dsmil_pool(feats, (const long long*)argmax, q_w, q_b, fcc_w, fcc_b, logits, A, B, a_raw ? a_raw : ws.raw,
                                ws.v, ws.vb, ws.lpart, ws.part, (int)n_tokens, dim, q_dim, n_classes, (hipStream_t)stream);
}

int rrt_dsmil_workspace_size(const rrt_dsmil_desc* desc, int64_t n_tokens, size_t* bytes) {
  if (!bytes) return RRT_E_INVALID;
  int rc = check_dsmil(desc, n_tokens);
  if (rc) return rc;
  HeadWs hw;
  rc = carve_dsmil_head(desc, n_tokens, nullptr, &hw, nullptr);
  if (rc) return rc;
  *bytes = hw.bytes;
  return RRT_OK;
}

int rrt_dsmil_forward_f32(const rrt_dsmil_desc* desc, const rrt_dsmil_weights* w, const float* x, float* logits,
                          float* classes_max, float* A, float* B, int64_t* argmax, int64_t n_tokens, void* workspace,
                          size_t workspace_bytes, void* stream) {
  if (!desc || !w || !x || !logits) return RRT_E_INVALID;
  int rc = check_dsmil(desc, n_tokens);
  if (rc) return rc;
  if (!w->emb_w || !w->icls_w || !w->q_w || !w->fcc_w) return RRT_E_INVALID;
  HeadWs hw;
  DsmilHeadWs ds;
  rc = carve_dsmil_head(desc, n_tokens, (char*)workspace, &hw, &ds);
  if (rc) return rc;
  if (!workspace || workspace_bytes < hw.bytes) return RRT_E_WORKSPACE;
  const int D = desc->enc.dim, K = desc->n_classes;
  long long* am = argmax ? (long long*)argmax : ds.argmax;
  float* cm = classes_max ? classes_max : ds.cmax;
  hipStream_t st = (hipStream_t)stream;
  // patch_to_emb follows enc.compute; everything behind the encoder -- instance classifier, q, scores, softmax, pooling,
  // fcc -- is fp32 in every mode: a 16-bit instance score could pick another critical instance
  bool p16 = false;
  rc = head_front_forward(head_front(desc), hw, x, w->emb_w, w->emb_b, &w->enc, nullptr, nullptr, 0, nullptr, /*tuning=*/false,
                          n_tokens, stream, &p16);
  if (rc) return rc;
  RRT_TRY(launch_instance_max(hw.y, w->icls_w, w->icls_b, nullptr, cm, am, ds.imax.pv, ds.imax.pi, (int)n_tokens, D, K, st));
  // (feats = the embedding: the bag stream reads it AFTER the encoder has run)
  return (int)launch_dsmil_pool(hw.emb, am, w->q_w, w->q_b, w->fcc_w, w->fcc_b, logits, A, B, ds.pool.raw, ds.pool.v, ds.pool.vb,
                                ds.pool.lpart, ds.pool.part, (int)n_tokens, D, desc->q_dim, K, st);
}

// ---- ABMIL / gated ABMIL / IBMIL / MeanMIL / MaxMIL: the mean pool and its adjoint, the deconfounder, the one-call forward
int rrt_bag_mean_workspace_size(int64_t n_tokens, int32_t dim, int32_t n_classes, size_t* bytes) {
  if (!bytes) return RRT_E_INVALID;
  int rc = check_bag_mean(n_tokens, dim, n_classes);
  if (rc) return rc;
  *bytes = carve_mean(n_tokens, dim, nullptr).bytes;
  return RRT_OK;
}

int rrt_bag_mean_f32(const float* y, const float* w, const float* b, float* logits, float* colmean, int64_t n_tokens,
                     int32_t dim, int32_t n_classes, void* workspace, size_t workspace_bytes, void* stream) {
  if (!y || !w || !logits) return RRT_E_INVALID;
  int rc = check_bag_mean(n_tokens, dim, n_classes);
  if (rc) return rc;
  if (!workspace || workspace_bytes < carve_mean(n_tokens, dim, nullptr).bytes) return RRT_E_WORKSPACE;
  MeanWs ws = carve_mean(n_tokens, dim, (char*)workspace);
  return (int)launch_bag_mean(y, w, b, logits, colmean, ws.part1, ws.part2, (int)n_tokens, dim, n_classes, (hipStream_t)stream);
}

int rrt_bag_mean_backward_f32(const float* d_logits, const float* colmean, const float* w, float* dy, float* dW, float* db,
                              int64_t n_tokens, int32_t dim, int32_t n_classes, void* stream) {
  if (!d_logits || (dy && !w) || (dW && !colmean) || (!dy && !dW && !db)) return RRT_E_INVALID;
  int rc = check_bag_mean(n_tokens, dim, n_classes);
  if (rc) return rc;
  return (int)launch_bag_mean_backward(d_logits, colmean, w, dy, dW, db, (int)n_tokens, dim, n_classes, (hipStream_t)stream);
}

int rrt_deconf_head_f32(const float* pooled, const float* conf, const float* q_w, const float* q_b, const float* k_w,
                        const float* k_b, const float* head_w, const float* head_b, float* logits, float* a, float* cf,
                        int32_t dim, int32_t n_conf, int32_t conf_dim, int32_t joint_dim, int32_t n_classes, void* stream) {
  if (!pooled || !conf || !q_w || !k_w || !head_w || !logits) return RRT_E_INVALID;
  int rc = check_deconf(dim, n_conf, conf_dim, joint_dim, n_classes);
  if (rc) return rc;
  return (int)launch_deconf_head(pooled, conf, q_w, q_b, k_w, k_b, head_w, head_b, logits, a, cf, dim, n_conf, conf_dim, joint_dim,
                                 n_classes, (hipStream_t)stream);
}

int rrt_bagmil_workspace_size(const rrt_bagmil_desc* desc, int64_t n_tokens, size_t* bytes) {
  if (!bytes) return RRT_E_INVALID;
  int rc = check_bagmil(desc, n_tokens);
  if (rc) return rc;
  HeadWs hw;
  rc = carve_bagmil_head(desc, n_tokens, nullptr, &hw, nullptr);
  if (rc) return rc;
  *bytes = hw.bytes;
  return RRT_OK;
}

int rrt_bagmil_forward_f32(const rrt_bagmil_desc* desc, const rrt_bagmil_weights* w, const float* x, float* logits, float* attn,
                           int32_t no_norm, float* pooled, int64_t* argmax, float* deconf_a, float* deconf_cf, int64_t n_tokens,
                           void* workspace, size_t workspace_bytes, void* stream) {
  if (!desc || !w || !x || !logits) return RRT_E_INVALID;
  int rc = check_bagmil(desc, n_tokens);
  if (rc) return rc;
  const int pool = desc->pool;
  const bool att = bagmil_attn(pool), gated = pool == RRT_BAGPOOL_ATTN_GATED, deconf = pool == RRT_BAGPOOL_ATTN_DECONF;
  if (!w->emb_w || !w->cls_w) return RRT_E_INVALID;
  if (att && (!w->a_w || !w->c_w || (gated && !w->b_w))) return RRT_E_INVALID;
  if (deconf && (!w->conf || !w->q_w || !w->k_w)) return RRT_E_INVALID;
  // an output the pool does not produce
  if ((attn && !att) || (pooled && pool == RRT_BAGPOOL_MAX) || (argmax && pool != RRT_BAGPOOL_MAX) ||
      ((deconf_a || deconf_cf) && !deconf))
    return RRT_E_INVALID;
  HeadWs hw;
  BagmilWs bws;
  rc = carve_bagmil_head(desc, n_tokens, (char*)workspace, &hw, &bws);
  if (rc) return rc;
  if (!workspace || workspace_bytes < hw.bytes) return RRT_E_WORKSPACE;
  const int D = desc->enc.dim, C = desc->n_classes;
  hipStream_t st = (hipStream_t)stream;
  const float* b_w = gated ? w->b_w : nullptr;
  bool p16 = false;
  rc = head_front_forward(head_front(desc), hw, x, w->emb_w, w->emb_b, &w->enc, att ? w->a_w : nullptr, b_w,
                          att ? desc->pool_hidden : 0, nullptr, /*tuning=*/false, n_tokens, stream, &p16);
  if (rc) return rc;
  // mean and max: fp32 in every mode (a 16-bit instance score could select another instance, as in DSMIL)
  if (pool == RRT_BAGPOOL_MEAN)
    return (int)launch_bag_mean(hw.y, w->cls_w, w->cls_b, logits, pooled, bws.mean.part1, bws.mean.part2, (int)n_tokens, D, C, st);
  if (pool == RRT_BAGPOOL_MAX)
    return (int)launch_instance_max(hw.y, w->cls_w, w->cls_b, nullptr, logits, argmax ? (long long*)argmax : bws.argmax,
                                    bws.imax.pv, bws.imax.pi, (int)n_tokens, D, C, st);
  // attention pools: the ABMIL pool of RRTMIL; the deconfounder variant takes its pooled row and no predictor
  float* pl = deconf ? (pooled ? pooled : bws.pooled) : pooled;
  rc = pool_predict(hw.y, w->a_w, w->a_b, b_w, w->b_b, w->c_w, w->c_b, deconf ? nullptr : w->cls_w, deconf ? nullptr : w->cls_b, pl,
                    deconf ? nullptr : logits, attn, no_norm, n_tokens, D, desc->pool_hidden, bagmil_pool_act(desc),
                    deconf ? 0 : C, gemm_precision(desc->enc.compute), bws.pool, st, p16 ? hw.y16 : nullptr,
                    p16 ? hw.pa16 : nullptr, (p16 && b_w) ? hw.pb16 : nullptr);
  if (rc || !deconf) return rc;
  return (int)launch_deconf_head(pl, w->conf, w->q_w, w->q_b, w->k_w, w->k_b, w->cls_w, w->cls_b, logits, deconf_a, deconf_cf, D,
                                 desc->deconf_k, desc->deconf_v, desc->deconf_j, C, st);
}

}  // extern "C"

// ------------------------------------------------------------------ batch-of-bags executor
#define RRT_EXEC_MAX_STREAMS 8
struct rrt_executor {
  rrt_encoder_desc desc;
  int n_streams;
  int device;
  hipStream_t streams[RRT_EXEC_MAX_STREAMS];
  void* ws[RRT_EXEC_MAX_STREAMS];
  size_t ws_bytes[RRT_EXEC_MAX_STREAMS];
  hipEvent_t fork, join[RRT_EXEC_MAX_STREAMS];
  rrt_phase_gate gate;
  // per workspace: (weights.version, compute) of the 16-bit weight images it holds (0 = none)
  uint64_t w16_version[RRT_EXEC_MAX_STREAMS];
  int w16_compute[RRT_EXEC_MAX_STREAMS];
  bool own_streams;      // false: the streams are the caller's (rrt_executor_create_on_streams), never destroyed here
  // slot 0 (its workspace) runs on whatever stream the CALLER passes: two calls from different streams must not overlap there
  hipEvent_t done0;
  bool has_done0;
};

extern "C" {

int rrt_executor_destroy(rrt_executor* ex) {
  if (!ex) return RRT_OK;
  (void)hipDeviceSynchronize();       // slot 0's workspace is used on the callers' streams
  for (int s = 0; s < ex->n_streams; ++s) {
    if (ex->streams[s]) (void)hipStreamSynchronize(ex->streams[s]);
    if (ex->ws[s]) (void)hipFree(ex->ws[s]);
    if (ex->join[s]) (void)hipEventDestroy(ex->join[s]);
    if (ex->streams[s] && ex->own_streams) (void)hipStreamDestroy(ex->streams[s]);
  }
  if (ex->fork) (void)hipEventDestroy(ex->fork);
  if (ex->done0) (void)hipEventDestroy(ex->done0);
  if (ex->gate.done) (void)hipEventDestroy(ex->gate.done);
  delete ex;
  return RRT_OK;
}

static int executor_create(const rrt_encoder_desc* desc, int32_t n_streams, int64_t max_tokens, void* const* user_streams,
                           rrt_executor** out) {
  if (!desc || !out || max_tokens <= 0) return RRT_E_INVALID;
  if (n_streams < 1 || n_streams > RRT_EXEC_MAX_STREAMS) return unsupported("executor: n_streams must be in [1,8]");
  size_t need = 0;
  int rc = rrt_encoder_workspace_size(desc, max_tokens, &need);
  if (rc) return rc;
  rrt_executor* ex = new rrt_executor();
  memset(ex, 0, sizeof(*ex));
  ex->desc = *desc;
  ex->n_streams = n_streams;
  ex->own_streams = user_streams == nullptr;
  hipError_t e = hipGetDevice(&ex->device);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&ex->fork, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&ex->gate.done, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&ex->done0, hipEventDisableTiming);
  for (int s = 0; s < n_streams && e == hipSuccess; ++s) {
    if (user_streams) {
      ex->streams[s] = (hipStream_t)user_streams[s];
    } else {
      static const char* smode = rrt_tune_env("RRT_EXEC_STREAMS");     // tuning build: how the executor's streams are made
      if (smode && smode[0] == 'p') {                                   // "prio": priorities spread over the device's range
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        const int span = lo - hi + 1;
        e = hipStreamCreateWithPriority(&ex->streams[s], hipStreamNonBlocking, hi + (span > 0 ? s % span : 0));
      } else {
        e = hipStreamCreateWithFlags(&ex->streams[s], hipStreamNonBlocking);
      }
    }
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ex->join[s], hipEventDisableTiming);
    if (e == hipSuccess) e = hipMalloc(&ex->ws[s], need);
    if (e == hipSuccess) ex->ws_bytes[s] = need;
  }
  if (e != hipSuccess) {
    rrt_executor_destroy(ex);
    return (int)e;
  }
  *out = ex;
  return RRT_OK;
}

int rrt_executor_create(const rrt_encoder_desc* desc, int32_t n_streams, int64_t max_tokens, rrt_executor** out) {
  return executor_create(desc, n_streams, max_tokens, nullptr, out);
}

int rrt_executor_create_on_streams(const rrt_encoder_desc* desc, int32_t n_streams, void* const* streams, int64_t max_tokens,
                                   rrt_executor** out) {
  if (!streams) return RRT_E_INVALID;
  if (n_streams < 1 || n_streams > RRT_EXEC_MAX_STREAMS) return unsupported("executor: n_streams must be in [1,8]");
  for (int s = 0; s < n_streams; ++s)
    for (int t = 0; t < s; ++t)
      if (streams[s] == streams[t]) return RRT_E_INVALID;      // the bags in flight need distinct streams
  return executor_create(desc, n_streams, max_tokens, streams, out);
}

int rrt_executor_forward(rrt_executor* ex, const rrt_encoder_weights* w, const rrt_bag* bags, int32_t n_bags,
                         void* stream) {
  if (!ex || !w || (n_bags > 0 && !bags) || n_bags < 0) return RRT_E_INVALID;
  if (n_bags == 0) return RRT_OK;
  if (n_bags > 65536) return unsupported("executor: more than 65536 bags in one call");
  // validate everything before the first launch: nothing runs if any bag is unsupported
  for (int i = 0; i < n_bags; ++i) {
    if (!bags[i].x || !bags[i].y || bags[i].x == bags[i].y) return RRT_E_INVALID;
    int rc = check_desc(&ex->desc, bags[i].n_tokens);
    if (rc) return rc;
  }
  // longest-processing-time-first onto the least loaded stream (cost ~ tokens); submission order within
  // a stream follows that order, so the big bags start first and the small ones fill the tail
  // Slots used by THIS call: one per four bags.  A fork / join costs every extra stream ~10 us of event waits and releases
  // the streams in lockstep, which pays off only when each stream then carries a few bags: with 2-4 bags per call four
  // streams were SLOWER than one (round 4, profiles/r04_final_bench_bags.txt: 4026-4368 vs 4480 slides/s), from 16 bags per
  // call on they win (4936-5062).  A call of < 8 bags is therefore plain launches on the caller's stream.  The kernels (and
  // bits) stay those of the executor's configured width: solo = (n_streams == 1) below does not depend on the call.
  int S = n_bags / 4;
  if (S < 1) S = 1;
  if (S > ex->n_streams) S = ex->n_streams;
  int order_buf[256];
  int* order = n_bags <= 256 ? order_buf : new int[n_bags];
  for (int i = 0; i < n_bags; ++i) order[i] = i;
  for (int i = 1; i < n_bags; ++i) {        // insertion sort, stable, descending n_tokens (n_bags is small)
    int v = order[i], j = i - 1;
    while (j >= 0 && bags[order[j]].n_tokens < bags[v].n_tokens) { order[j + 1] = order[j]; --j; }
    order[j + 1] = v;
  }
  hipStream_t caller = (hipStream_t)stream;
  // Slot 0 runs on the CALLER's stream, slots 1 .. S-1 on the executor's.  Round 4: with all S slots on own streams the
  // caller's stream sat through the whole call with S barrier packets (the join) at its head -- a (S+1)-th active hardware
  // queue next to the S that carry bags.  At S = 4 that is five queues on four pipes: 4.3-4.45 k slides/s where the same
  // launches on four queues give 5.07-5.10 k (tools/bench_bags.py with the join compiled out; the five-stream bench line
  // shows the same loss).  Now the join's waits sit BEHIND the caller stream's own share of the bags, the fork only
  // concerns the other slots, and a one-stream executor is plain launches on the caller's stream.
  hipStream_t sts[RRT_EXEC_MAX_STREAMS];
  sts[0] = caller;
  for (int s = 1; s < S; ++s) sts[s] = ex->streams[s];
  hipError_t e = hipSuccess;
  // (the previous call may have come from ANOTHER stream: its slot-0 work, on that stream, owns workspace 0 until it is done)
  if (ex->has_done0) RRT_TRY(hipStreamWaitEvent(caller, ex->done0, 0));
  static const bool no_fork = rrt_tune_env("RRT_EXEC_NOFORK") != nullptr;      // (bisecting, tuning build only)
  if (S > 1 && !no_fork) {
    e = hipEventRecord(ex->fork, caller);
    for (int s = 1; s < S && e == hipSuccess; ++s) e = hipStreamWaitEvent(sts[s], ex->fork, 0);
  }
  int rc = (int)e;
  int64_t load[RRT_EXEC_MAX_STREAMS] = {0};
  // phase gate (the R-MSA cores of the bags in flight take turns): opt-in, RRT_GATE=1.  It paid +1.5 % at two bags in
  // flight with the round-1 kernels; with the round-2 kernels free-running streams are faster at every S (configs[4]
  // mix, bf16: 7.72 k vs 7.49 k slides/s; fp32: 3.74 k vs 3.68 k)
  static const bool gate_on = rrt_tune_env("RRT_GATE") != nullptr;
  const bool gated = S == 2 && gate_on;
  // tuning build: RRT_EXEC_STAGGER=1 -> only the FIRST bag of every stream goes through the gate, so that the streams of a
  // call start one R-MSA core apart instead of in lockstep (the fork releases them together)
  static const bool stagger = rrt_tune_env("RRT_EXEC_STAGGER") != nullptr;
  if (stagger) ex->gate.armed = false;
  for (int k = 0; k < n_bags && rc == RRT_OK; ++k) {
    const rrt_bag& b = bags[order[k]];
    int s = 0;
    for (int t = 1; t < S; ++t)
      if (load[t] < load[s]) s = t;
    load[s] += b.n_tokens;
    size_t need = 0;
    rc = rrt_encoder_workspace_size(&ex->desc, b.n_tokens, &need);
    if (rc) break;
    if (need > ex->ws_bytes[s]) {            // grow: the only host synchronisation in this call
      e = hipStreamSynchronize(sts[s]);
      if (e == hipSuccess) e = hipFree(ex->ws[s]);
      ex->ws[s] = nullptr;
      ex->ws_bytes[s] = 0;
      if (e == hipSuccess) e = hipMalloc(&ex->ws[s], need);
      if (e != hipSuccess) { rc = (int)e; break; }
      ex->ws_bytes[s] = need;
      ex->w16_version[s] = 0;
    }
    rrt_encoder_desc d = ex->desc;
    d.solo = ex->n_streams == 1;
    d.weights16_valid = w->version != 0 && ex->w16_version[s] == w->version && ex->w16_compute[s] == d.compute;
    rc = encoder_forward(&d, w, b.x, b.y, b.n_tokens, ex->ws[s], ex->ws_bytes[s], sts[s], nullptr,
                         (gated || (stagger && k < S)) ? &ex->gate : nullptr);
    ex->w16_version[s] = rc == RRT_OK ? w->version : 0;
    ex->w16_compute[s] = d.compute;
  }
  // join even after an error so the caller's stream stays ordered after whatever was enqueued
  static const bool no_join = rrt_tune_env("RRT_EXEC_NOJOIN") != nullptr;      // (bisecting, tuning build only)
  for (int s = 1; s < S && !no_join; ++s) {
    hipError_t j = hipEventRecord(ex->join[s], sts[s]);
    if (j == hipSuccess) j = hipStreamWaitEvent(caller, ex->join[s], 0);
    if (rc == RRT_OK && j != hipSuccess) rc = (int)j;
  }
  if (hipEventRecord(ex->done0, caller) == hipSuccess) ex->has_done0 = true;
  if (order != order_buf) delete[] order;
  return rc;
}

}  // extern "C"

// ------------------------------------------------------------------ row f2 building blocks (backward stages)
extern "C" {

int rrt_region_attention_backward_workspace_size(int32_t n_regions, int32_t P, int32_t dim, int32_t heads,
                                                 int32_t epeg_k, size_t* bytes) {
  if (!bytes || n_regions <= 0 || P <= 0 || dim <= 0 || heads <= 0) return RRT_E_INVALID;
  *bytes = attn_bwd_workspace(n_regions, P, dim, heads, epeg_k);
  return RRT_OK;
}

int rrt_region_attention_backward_f32(const float* qkv, const float* pe_w, const float* o, const float* d_o,
                                      float* d_qkv, float* d_pe_w, int32_t n_regions, int32_t P, int32_t dim,
                                      int32_t heads, int32_t epeg_k, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  if (!qkv || !o || !d_o || !d_qkv || n_regions <= 0 || P <= 0 || dim <= 0 || heads <= 0) return RRT_E_INVALID;
  const int ek = pe_w ? epeg_k : 0;
  if (ek > 0 && ek % 2 == 0) return unsupported("epeg_k must be odd");
  if (!attn_bwd_supported(P, dim, heads, ek))
    return unsupported("attention backward: needs a head dim that is a multiple of 16 up to 256 with epeg_k <= 63 (any P), "
                       "or no EPEG, P <= 128 and a head dim that is a multiple of 4");
  if (!workspace || workspace_bytes < attn_bwd_workspace(n_regions, P, dim, heads, ek)) return RRT_E_WORKSPACE;
  return (int)launch_attention_backward(qkv, pe_w, o, d_o, d_qkv, d_pe_w, (float*)workspace, n_regions, P, dim,
                                        heads, ek, (hipStream_t)stream);
}

int rrt_layernorm_backward_f32(const float* dy, const float* x, const float* gamma, const float* add, float* dx,
                               float* dgamma_dbeta, int64_t L, int32_t dim, const rrt_grid* g, void* workspace,
                               size_t workspace_bytes, void* stream) {
  if (!dy || !x || !gamma || !dx || !dgamma_dbeta || L <= 0 || dim <= 0 || dim % 4) return RRT_E_INVALID;
  if (dim > 2048) return unsupported("dim > 2048");
  if (g && g->L != L) return RRT_E_INVALID;
  if (!workspace || workspace_bytes < ln_bwd_workspace(dim)) return RRT_E_WORKSPACE;
  GridDev gd{};
  if (g) gd = to_dev(*g);
  return (int)launch_ln_backward(dy, x, gamma, add, dx, dgamma_dbeta, (float*)workspace, (int)L, dim,
                                 g ? &gd : nullptr, (hipStream_t)stream);
}

// ---- stage entry points of the ablation kernels (peg.hip, epeg_variants.hip): one launcher each, arguments checked
namespace {
int check_peg_stage(int64_t N, int32_t dim, int32_t k) {
  if (N <= 0 || N > (int64_t)4000000 || dim <= 0) return RRT_E_INVALID;
  if (dim % 4) return unsupported("peg: dim must be a multiple of 4");
  if (k <= 0 || k % 2 == 0 || k > 11) return unsupported("peg_k must be odd and <= 11");
  return RRT_OK;
}
int check_epeg_stage(int32_t n_regions, int32_t P, int32_t dim, int32_t heads, int32_t k) {
  if (n_regions <= 0 || P <= 0 || dim <= 0 || heads <= 0) return RRT_E_INVALID;
  if (dim % 4) return unsupported("epeg ablations: dim must be a multiple of 4");
  if (dim % heads) return unsupported("n_heads must divide dim");
  if (k <= 0 || k % 2 == 0) return unsupported("epeg_k must be odd");
  if (k > 63) return unsupported("epeg ablations: epeg_k <= 63");
  if ((int64_t)n_regions * P > (int64_t)4000000 || n_regions > 65535) return unsupported("epeg ablations: more than 65535 regions or 4e6 slots");
  return RRT_OK;
}
size_t scoremap_scratch_bytes(int n_regions, int P, int heads, int k, int backward) {
  if (!backward) return attn_scoremap_scratch_floats(n_regions, P, heads, k, 1) * sizeof(float);
  return (attn_scoremap_scratch_floats(n_regions, P, heads, k, 3) + (size_t)n_regions * heads * k * k) * sizeof(float);
}
}  // namespace

int rrt_peg_f32(const float* x, const float* const* w, const float* const* b, float* y, int64_t N, int32_t dim, int32_t k,
                int32_t conv_1d, int32_t ppeg, void* stream) {
  if (!x || !y || !w || !w[0] || (ppeg && (!w[1] || !w[2]))) return RRT_E_INVALID;
  const int rc = check_peg_stage(N, dim, k);
  if (rc) return rc;
  const float* nob[3] = {nullptr, nullptr, nullptr};
  return (int)launch_peg(x, w, b ? b : nob, y, (int)N, dim, k, conv_1d != 0, ppeg != 0, (hipStream_t)stream);
}

int rrt_peg_backward_workspace_size(int64_t N, int32_t dim, int32_t k, int32_t ppeg, size_t* bytes) {
  if (!bytes) return RRT_E_INVALID;
  const int rc = check_peg_stage(N, dim, k);
  if (rc) return rc;
  *bytes = peg_bwd_workspace((int)N, dim, k, ppeg != 0);
  return RRT_OK;
}

int rrt_peg_backward_f32(const float* x, const float* dy, const float* const* w, float* dx, float* const* dw, float* const* db,
                         int64_t N, int32_t dim, int32_t k, int32_t conv_1d, int32_t ppeg, void* workspace,
                         size_t workspace_bytes, void* stream) {
  if (!x || !dy || !dx || !w || !dw || !w[0] || !dw[0] || (ppeg && (!w[1] || !w[2] || !dw[1] || !dw[2]))) return RRT_E_INVALID;
  const int rc = check_peg_stage(N, dim, k);
  if (rc) return rc;
  if (!workspace || workspace_bytes < peg_bwd_workspace((int)N, dim, k, ppeg != 0)) return RRT_E_WORKSPACE;
  float* const nodb[3] = {nullptr, nullptr, nullptr};
  return (int)launch_peg_backward(x, dy, w, dx, dw, db ? db : nodb, (int)N, dim, k, conv_1d != 0, ppeg != 0, workspace,
                                  (hipStream_t)stream);
}

int rrt_attn_scoremap_scratch_size(int32_t n_regions, int32_t P, int32_t heads, int32_t k, int32_t backward, size_t* bytes) {
  if (!bytes) return RRT_E_INVALID;
  const int rc = check_epeg_stage(n_regions, P, 4 * heads, heads, k);
  if (rc) return rc;
  *bytes = scoremap_scratch_bytes(n_regions, P, heads, k, backward != 0);
  return RRT_OK;
}

int rrt_attn_scoremap_f32(const float* qkv, const float* pe_w, float* o, int32_t n_regions, int32_t P, int32_t dim,
                          int32_t heads, int32_t k, void* scratch, size_t scratch_bytes, void* stream) {
  if (!qkv || !pe_w || !o) return RRT_E_INVALID;
  const int rc = check_epeg_stage(n_regions, P, dim, heads, k);
  if (rc) return rc;
  if (((size_t)k * k + 4 * (size_t)P) * sizeof(float) > 160 * 1024) return unsupported("attn_scoremap: region too large");
  const size_t need = scoremap_scratch_bytes(n_regions, P, heads, k, 0);
  if (need && (!scratch || scratch_bytes < need)) return RRT_E_WORKSPACE;
  return (int)launch_attn_scoremap(qkv, pe_w, o, need ? (float*)scratch : nullptr, n_regions, P, dim, heads, k,
                                   (hipStream_t)stream);
}

int rrt_attn_scoremap_backward_f32(const float* qkv, const float* pe_w, const float* d_o, float* d_qkv, float* d_pe_w,
                                   int32_t n_regions, int32_t P, int32_t dim, int32_t heads, int32_t k, void* scratch,
                                   size_t scratch_bytes, void* stream) {
  if (!qkv || !pe_w || !d_o || !d_qkv || !d_pe_w) return RRT_E_INVALID;
  const int rc = check_epeg_stage(n_regions, P, dim, heads, k);
  if (rc) return rc;
  if (((size_t)k * k + 4 * (size_t)P) * sizeof(float) > 160 * 1024) return unsupported("attn_scoremap: region too large");
  if (!scratch || scratch_bytes < scoremap_scratch_bytes(n_regions, P, heads, k, 1)) return RRT_E_WORKSPACE;
  return (int)launch_attn_scoremap_backward(qkv, pe_w, d_o, d_qkv, d_pe_w, (float*)scratch, n_regions, P, dim, heads, k,
                                            (hipStream_t)stream);
}

int rrt_value_pe_f32(const float* qkv, const float* w, const float* bias, float* pe, int32_t n_regions, int32_t P, int32_t s,
                     int32_t dim, int32_t heads, int32_t k, int32_t two_d, void* stream) {
  if (!qkv || !w || !pe || s <= 0) return RRT_E_INVALID;
  const int rc = check_epeg_stage(n_regions, P, dim, heads, k);
  if (rc) return rc;
  if ((int64_t)s * s != P) return unsupported("value epeg: the region must be an s x s image");
  return (int)launch_value_pe(qkv, w, bias, pe, n_regions, P, s, dim, heads, k, two_d != 0, (hipStream_t)stream);
}

int rrt_value_pe_backward_f32(const float* d_pe, const float* qkv, const float* vsub, const float* w, float* d_qkv, float* d_w,
                              float* d_b, int32_t n_regions, int32_t P, int32_t s, int32_t dim, int32_t heads, int32_t k,
                              int32_t two_d, void* stream) {
  if (!d_pe || !qkv || !w || !d_qkv || !d_w || s <= 0) return RRT_E_INVALID;
  const int rc = check_epeg_stage(n_regions, P, dim, heads, k);
  if (rc) return rc;
  if ((int64_t)s * s != P) return unsupported("value epeg: the region must be an s x s image");
  if ((size_t)2 * P * sizeof(float) > 160 * 1024) return unsupported("value epeg backward: region too large");
  return (int)launch_value_pe_backward(d_pe, qkv, vsub, w, d_qkv, d_w, d_b, n_regions, P, s, dim, heads, k, two_d != 0,
                                       (hipStream_t)stream);
}

int rrt_reduce_partials_f32(const float* part, float* out, float* out_tr, int32_t S, int64_t n, int64_t split,
                            int32_t tr_dim, int32_t tr_k, int32_t deferred, int32_t copies, void* stream) {
  if (!part || !out || S <= 0 || n <= 0 || S > (1 << 20)) return RRT_E_INVALID;
  if (out_tr && (split < 0 || split % 4 || split > n || tr_dim <= 0 || tr_k <= 0 || n - split != (int64_t)tr_dim * tr_k))
    return RRT_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  if (!deferred) {
    if (out_tr) return (int)launch_reduce_partials_scatter(part, out, S, (size_t)n, (size_t)split, out_tr, tr_dim, tr_k, st);
    return (int)launch_reduce_partials(part, out, S, (size_t)n, st);
  }
  if (copies < 1 || copies > REDUCE_MAX_JOBS) return RRT_E_INVALID;
  ReduceJobs rj{};
  for (int c = 0; c < copies; ++c) {
    RRT_TRY(reduce_or_defer(&rj, part, out + (size_t)c * n, S, (size_t)n, st, (size_t)(out_tr ? split : 0),
                            out_tr ? out_tr + (size_t)c * tr_dim * tr_k : nullptr, tr_dim, tr_k));
  }
  return (int)launch_reduce_jobs(rj, st);
}

int rrt_linear_backward_workspace_size(int64_t M, int32_t N, int32_t K, size_t* bytes) {
  if (!bytes || M <= 0 || N <= 0 || K <= 0 || M > (int64_t)16000000) return RRT_E_INVALID;
  *bytes = linear_bwd_workspace((int)M, N, K);
  return RRT_OK;
}

int rrt_linear_backward_f32(const float* dY, const float* X, const float* W, float* dX, float* dW, float* db,
                            int64_t M, int32_t N, int32_t K, int32_t compute, void* workspace,
                            size_t workspace_bytes, void* stream) {
  if (!dY || M <= 0 || N <= 0 || K <= 0 || M > (int64_t)16000000) return RRT_E_INVALID;
  if ((dX && !W) || (dW && !X)) return RRT_E_INVALID;
  if (dX && N % 32) return unsupported("linear backward: N must be a multiple of 32 for dX");
  if (compute < 0 || compute > 2) return unsupported("compute must be RRT_COMPUTE_F32/BF16/F16");
  if (!workspace || workspace_bytes < linear_bwd_workspace((int)M, N, K)) return RRT_E_WORKSPACE;
  return (int)launch_linear_backward(dY, X, W, dX, dW, db, (int)M, N, K, compute, workspace, (hipStream_t)stream);
}

}  // extern "C"

// ------------------------------------------------------------------ row f2: training forward + backward
namespace {

struct Stash {
  float *u[RRT_MAX_RMSA_LAYERS], *qkv[RRT_MAX_RMSA_LAYERS], *o[RRT_MAX_RMSA_LAYERS], *xout[RRT_MAX_RMSA_LAYERS];
  float *mean_rstd, *logits, *wdisp, *rep, *rep_qkv, *rep_o, *rep2, *x2, *v8, *hid;
  // ffn = 1: per TransLayer (index n_rmsa_layers = CR-MSA's) LN2 output, fc1 pre-activation, layer output;
  // xcr = CR-MSA's output before its FFN; hscr = one scratch for act(hpre)
  float *ffn_u[RRT_MAX_RMSA_LAYERS + 1], *ffn_hpre[RRT_MAX_RMSA_LAYERS + 1], *xf[RRT_MAX_RMSA_LAYERS + 1];
  float *xcr, *hscr, *xp;     // xp: output of the PEG / PPEG stage (pos != none)
  float *pe[RRT_MAX_RMSA_LAYERS];   // value-EPEG ablations: the conv's output per layer
  float *smap;                // 2-D 'attn' EPEG: score-map scratch of the forward (large regions only)
  size_t bytes;
};

Stash carve_stash(const rrt_encoder_desc& d, int64_t N, const rrt_grid& g, const rrt_grid& g8, char* base) {
  Stash s{};
  Arena a{base};
  const size_t D = d.dim, Np = (size_t)g.H * g.H, Np8 = (size_t)g8.H * g8.H;
  const size_t R8 = (size_t)g8.regions_side * g8.regions_side, k = d.crmsa_k;
  for (int l = 0; l < d.n_rmsa_layers; ++l) {
    s.u[l] = a.take(Np * D);
    s.qkv[l] = a.take(Np * 3 * D);
    s.o[l] = a.take(Np * D);
    s.xout[l] = a.take((size_t)N * D);
    if (d.epeg && d.epeg_type != RRT_EPEG_ATTN) s.pe[l] = a.take(Np * D);
  }
  if (d.n_rmsa_layers > 0 && d.epeg && d.epeg_2d && d.epeg_type == RRT_EPEG_ATTN) {
    const size_t sm = attn_scoremap_scratch_floats(g.regions_side * g.regions_side, g.s * g.s, d.n_heads, d.epeg_k, 1);
    if (sm) s.smap = a.take(sm);
  }
  if (d.cr_msa) {
    s.mean_rstd = a.take((size_t)N * 2);
    s.logits = a.take(Np8 * k);
    s.wdisp = a.take(Np8 * k);
    s.rep = a.take(k * R8 * D);
    s.rep_qkv = a.take(k * R8 * 3 * D);
    s.rep_o = a.take(k * R8 * D);
    s.rep2 = a.take(k * R8 * D);
    if (d.crmsa_mlp) {
      s.v8 = a.take(Np8 * D);
      s.hid = a.take(Np8 * (D / 4));
    }
  }
  s.x2 = a.take((size_t)N * D);
  if (d.ffn) {
    const int nl = d.n_rmsa_layers + (d.cr_msa ? 1 : 0);
    for (int l = 0; l < nl; ++l) {
      const int idx = l < d.n_rmsa_layers ? l : RRT_MAX_RMSA_LAYERS;
      s.ffn_u[idx] = a.take((size_t)N * D);
      s.ffn_hpre[idx] = a.take((size_t)N * d.ffn_hidden);
      s.xf[idx] = a.take((size_t)N * D);
    }
    if (d.cr_msa) s.xcr = a.take((size_t)N * D);
    s.hscr = a.take((size_t)N * d.ffn_hidden);
  }
  if (d.pos) s.xp = a.take((size_t)N * D);
  s.bytes = a.bytes();
  return s;
}

struct BwdWs {
  float *dx2, *dxa, *dxb, *dz, *dO, *dqkv, *lnpart, *attnpart, *dWd, *dC, *dlg, *Cw, *d_rep2, *d_rep_o,
      *d_rep_qkv, *d_rep, *rows, *dxpart, *th, *dhid, *dvphi, *w1t, *tnscratch, *fh, *fdh, *fdu, *attnpart_cr, *dpe, *smap;
  char *lin, *pegws;
  float* tappart[RRT_MAX_RMSA_LAYERS];     // the EPEG taps' partials of each layer (summed by the deferred reduce launch)
  size_t lnpart_stride;                    // lnpart holds one partial buffer per LayerNorm backward of the pass
  float *wt_qkv[RRT_MAX_RMSA_LAYERS], *wt_proj[RRT_MAX_RMSA_LAYERS], *wt_cr_qkv, *wt_cr_proj;   // W^T images, made in one launch
  size_t bytes;
};

BwdWs carve_bwd(const rrt_encoder_desc& d, int64_t N, const rrt_grid& g, const rrt_grid& g8, char* base) {
  BwdWs w{};
  Arena a{base};
  const size_t D = d.dim, Np = (size_t)g.H * g.H, Np8 = (size_t)g8.H * g8.H;
  const size_t R8 = (size_t)g8.regions_side * g8.regions_side, k = d.crmsa_k;
  w.dx2 = a.take((size_t)N * D);
  w.dxa = a.take((size_t)N * D);
  w.dxb = a.take((size_t)N * D);
  w.lnpart_stride = align_up(ln_bwd_workspace((int)D), 256) / sizeof(float);
  w.lnpart = a.take(w.lnpart_stride * (size_t)(2 * (d.n_rmsa_layers + 1) + 1));      // final + (norm, norm2) per layer + CR-MSA's norm2
  size_t lin = 0;
  if (d.n_rmsa_layers > 0) {
    w.dz = a.take(Np * D);
    w.dO = a.take(Np * D);
    w.dqkv = a.take(Np * 3 * D);
    const int R = g.regions_side * g.regions_side;
    const bool e2d = d.epeg && d.epeg_2d && d.epeg_type == RRT_EPEG_ATTN, evalue = d.epeg && d.epeg_type != RRT_EPEG_ATTN;
    if (e2d) {       // 2-D 'attn' EPEG: its own backward kernel (three [P, P] maps per (region, head) + the tap partials)
      w.smap = a.take(attn_scoremap_scratch_floats(R, g.s * g.s, d.n_heads, d.epeg_k, 3) + (size_t)R * d.n_heads * d.epeg_k * d.epeg_k);
      w.attnpart = a.take(64);
    } else {
      w.attnpart = a.take(attn_bwd_workspace(R, g.s * g.s, (int)D, d.n_heads, (d.epeg && !evalue) ? d.epeg_k : 0) / sizeof(float));
      if (d.epeg && !evalue)
        for (int li = 0; li < d.n_rmsa_layers; ++li) w.tappart[li] = a.take((size_t)R * d.n_heads * d.epeg_k);
    }
    if (evalue) w.dpe = a.take(Np * D);
    lin = linear_bwd_workspace((int)Np, 3 * (int)D, (int)D);
    const size_t l2 = linear_bwd_workspace((int)Np, (int)D, (int)D);
    if (l2 > lin) lin = l2;
  }
  if (d.cr_msa) {
    w.dWd = a.take(Np8 * k);
    w.dC = a.take(Np8 * k);
    w.dlg = a.take(Np8 * k);
    w.Cw = a.take(Np8 * k);
    w.d_rep2 = a.take(k * R8 * D);
    w.d_rep_o = a.take(k * R8 * D);
    w.d_rep_qkv = a.take(k * R8 * 3 * D);
    w.d_rep = a.take(k * R8 * D);
    w.rows = a.take((2 + k) * D);
    w.dxpart = a.take(crmsa_bwd_dx_workspace((int)D, (int)k) / sizeof(float));
    if (d.crmsa_mlp) {
      w.th = a.take(Np8 * (D / 4));
      w.dhid = a.take(Np8 * (D / 4));
      w.dvphi = a.take(Np8 * D);
      w.w1t = a.take(D * (D / 4));
      const size_t a1 = linear_bwd_workspace((int)Np8, (int)(D / 4), (int)D);     // dW1 partials dominate
      const size_t a2 = linear_bwd_workspace((int)Np8, (int)k, (int)(D / 4));
      w.tnscratch = a.take((a1 > a2 ? a1 : a2) / sizeof(float));
    }
    // attnpart is shared by the R-MSA layers' and CR-MSA's attention backward: the larger of the two geometries
    // (a small bag's R-MSA partials can be smaller than what CR-MSA's 64-token regions need)
    w.attnpart_cr = a.take(attn_bwd_workspace((int)k, (int)R8, (int)D, d.crmsa_heads, 0) / sizeof(float));
    const size_t l3 = linear_bwd_workspace((int)(k * R8), 3 * (int)D, (int)D);
    if (l3 > lin) lin = l3;
  }
  if (d.ffn) {
    w.fh = a.take((size_t)N * d.ffn_hidden);
    w.fdh = a.take((size_t)N * d.ffn_hidden);
    w.fdu = a.take((size_t)N * D);
    const size_t f1 = linear_bwd_workspace((int)N, (int)D, d.ffn_hidden), f2 = linear_bwd_workspace((int)N, d.ffn_hidden, (int)D);
    if (f1 > lin) lin = f1;
    if (f2 > lin) lin = f2;
  }
  w.lin = a.take<char>(lin ? lin : 256);
  if (d.pos) w.pegws = a.take<char>(peg_bwd_workspace((int)N, (int)D, d.peg_k, d.pos == RRT_POS_PPEG));
  for (int li = 0; li < d.n_rmsa_layers; ++li) {
    w.wt_qkv[li] = a.take(3 * D * D);
    w.wt_proj[li] = a.take(D * D);
  }
  if (d.cr_msa) {
    w.wt_cr_qkv = a.take(3 * D * D);
    w.wt_cr_proj = a.take(D * D);
  }
  w.bytes = a.bytes();
  return w;
}

int check_train(const rrt_encoder_desc* d, int64_t N, rrt_grid* g, rrt_grid* g8) {
  int rc = check_desc(d, N);
  if (rc) return rc;
  if (d->compute == RRT_COMPUTE_F32X3) return unsupported("training: RRT_COMPUTE_F32X3 is an inference mode (train in F32 or under autocast)");
  if (d->dim > 1024) return unsupported("training: dim > 1024");
  rc = region_grids(d, N, g, g8);
  if (rc) return rc;
  if (d->n_rmsa_layers > 0) {
    const bool e2d = d->epeg && d->epeg_2d && d->epeg_type == RRT_EPEG_ATTN, evalue = d->epeg && d->epeg_type != RRT_EPEG_ATTN;
    // (the 2-D 'attn' EPEG has its own backward kernel, any head dim; the value variants run the plain attention backward)
    if (!e2d && !attn_bwd_supported(g->s * g->s, d->dim, d->n_heads, (d->epeg && !evalue) ? d->epeg_k : 0))
      return unsupported("training: the R-MSA attention backward needs a head dim that is a multiple of 16 up to 256 (any region size, epeg_k <= 63); other head dims (not a multiple of 16, or above 256) only without EPEG on regions of <= 128 tokens, or with epeg_2d");
  }
  if (d->cr_msa) {
    const int R8 = g8->regions_side * g8->regions_side;
    if (!attn_bwd_supported(R8, d->dim, d->crmsa_heads, 0))
      return unsupported("training: CR-MSA's inner attention needs a head dim that is a multiple of 4");
  }
  return RRT_OK;
}

}  // namespace

extern "C" {

int rrt_encoder_train_sizes(const rrt_encoder_desc* desc, int64_t n_tokens, size_t* stash_bytes,
                            size_t* backward_workspace_bytes) {
  if (!desc || !stash_bytes || !backward_workspace_bytes) return RRT_E_INVALID;
  rrt_grid g{}, g8{};
  int rc = check_train(desc, n_tokens, &g, &g8);
  if (rc) return rc;
  *stash_bytes = carve_stash(*desc, n_tokens, g, g8, nullptr).bytes;
  *backward_workspace_bytes = carve_bwd(*desc, n_tokens, g, g8, nullptr).bytes;
  return RRT_OK;
}

namespace {
constexpr int DROP_LAYER_CRMSA = 100;
// stochastic depth (TransLayer.drop_path, rrt.py:102,125,129): per-call multipliers of the residual branches,
// host array [2][RRT_MAX_RMSA_LAYERS + 1] = {attention branches, FFN branches}, index n_rmsa_layers = CR-MSA's
struct Branch {
  float attn[RRT_MAX_RMSA_LAYERS + 1], ffn[RRT_MAX_RMSA_LAYERS + 1];
};
int make_branch(const float* bs, Branch* b) {
  for (int i = 0; i <= RRT_MAX_RMSA_LAYERS; ++i) {
    b->attn[i] = bs ? bs[i] : 1.0f;
    b->ffn[i] = bs ? bs[RRT_MAX_RMSA_LAYERS + 1 + i] : 1.0f;
    if (!(b->attn[i] >= 0.f) || !(b->ffn[i] >= 0.f)) return RRT_E_INVALID;
  }
  return RRT_OK;
}
}  // namespace

// ---- the GEMM family's form report and its stage entry (tests/test_linear_form_matrix.py, test_linear_form_grid_cpu.py)
namespace {
// the fields of a LinearEpilogue that plan_linear looks at, for an RRT_LINEAR_EPI_* value; `set` stands for "this pointer is
// given" (never followed)
int epilogue_kind(int32_t epilogue, int32_t compute, int32_t operands, int32_t K, int32_t solo, bool zero64, LinearEpilogue* ep) {
  static const float set_f = 0.f;
  static int set_i = 0;
  if (epilogue < RRT_LINEAR_EPI_PLAIN || epilogue > RRT_LINEAR_EPI_DROP) return RRT_E_INVALID;
  if (operands == RRT_LINEAR_OPS_F32) {
    if (compute < 0 || compute > 2) return unsupported("linear: fp32 operands take RRT_COMPUTE_F32 / BF16 / F16");
  } else if (operands == RRT_LINEAR_OPS_16) {
    if (compute != RRT_COMPUTE_BF16 && compute != RRT_COMPUTE_F16) return unsupported("linear: 16-bit images take RRT_COMPUTE_BF16 / F16");
  } else if (operands == RRT_LINEAR_OPS_SPLIT) {
    if (compute != RRT_COMPUTE_F32X3) return unsupported("linear: split images take RRT_COMPUTE_F32X3");
  } else {
    return RRT_E_INVALID;
  }
  if (K % (operands == RRT_LINEAR_OPS_16 ? 64 : 32))
    return unsupported("linear: K must be a multiple of 32 (16-bit images: 64)");
  ep->prec = operands == RRT_LINEAR_OPS_SPLIT ? 0 : compute;
  ep->act = epilogue == RRT_LINEAR_EPI_ACT ? RRT_ACT_RELU : RRT_ACT_NONE;
  ep->resid = (epilogue == RRT_LINEAR_EPI_UNPART || epilogue == RRT_LINEAR_EPI_UNPART_DROP) ? &set_f : nullptr;
  ep->drop_on = epilogue == RRT_LINEAR_EPI_DROP || epilogue == RRT_LINEAR_EPI_UNPART_DROP;
  ep->solo = solo != 0;
  ep->zero64 = zero64 ? &set_i : nullptr;
  return RRT_OK;
}
}  // namespace

int rrt_linear_plan(int64_t M, int32_t N, int32_t K, int32_t compute, int32_t operands, int32_t epilogue, int32_t solo,
                    int32_t zero64, int32_t* plan) {
  if (!plan || M <= 0 || M > 0x7FFFFFFF || N <= 0 || K <= 0) return RRT_E_INVALID;
  for (int i = 0; i < RRT_LINEAR_PLAN_INTS; ++i) plan[i] = 0;
  LinearEpilogue ep{};
  int rc = epilogue_kind(epilogue, compute, operands, K, solo, zero64 != 0, &ep);
  if (rc) return rc;
  LinearPlan pl{};
  if (plan_linear(operands, (int)M, N, K, ep, &pl) != hipSuccess)
    return unsupported("linear: the launcher of this operand kind refuses the combination (K % 32 / % 64, dropout outside exact "
                       "fp32 or with an activation, activation on split images)");
  const int v[RRT_LINEAR_PLAN_INTS] = {pl.kernel, pl.mt, pl.nt, pl.cap, pl.ntiles, pl.grid, pl.defer, pl.kg, pl.drop, pl.mode, pl.prec, 0};
  for (int i = 0; i < RRT_LINEAR_PLAN_INTS; ++i) plan[i] = v[i];
  return RRT_OK;
}

int rrt_debug_linear_f32(const void* A, const void* B, const float* bias, const float* resid, float* C, int64_t M, int32_t N,
                         int32_t K, const rrt_grid* g, int32_t operands, int32_t compute, int32_t q_cols, float q_scale,
                         int32_t act, int32_t solo, float drop_p, uint64_t drop_seed, int32_t drop_layer, int32_t* zero64,
                         void* stream) {
  if (!A || !B || !C || M <= 0 || M > 0x7FFFFFFF || N <= 0 || K <= 0 || (resid && !g)) return RRT_E_INVALID;
  if (q_cols < 0 || q_cols > N || act < RRT_ACT_NONE || act > RRT_ACT_SIGMOID || drop_layer < 0) return RRT_E_INVALID;
  DropCfg dc{};
  if (make_drop(drop_p, &dc)) return RRT_E_INVALID;
  if (resid && act) return unsupported("linear: the un-partition epilogue has no activation");
  const bool drop_on = dc.thresh != 0;
  const int32_t epilogue = drop_on ? (resid ? RRT_LINEAR_EPI_UNPART_DROP : RRT_LINEAR_EPI_DROP)
                           : resid ? RRT_LINEAR_EPI_UNPART : act ? RRT_LINEAR_EPI_ACT : RRT_LINEAR_EPI_PLAIN;
  if (drop_on && act) return unsupported("linear: the dropout epilogue has no activation");
  LinearEpilogue ep{};
  int rc = epilogue_kind(epilogue, compute, operands, K, solo, zero64 != nullptr, &ep);
  if (rc) return rc;
  ep.act = act;
  ep.bias = bias;
  ep.q_cols = q_cols;
  ep.q_scale = q_scale;
  ep.resid = resid;
  ep.zero64 = zero64;
  if (resid) {
    ep.g = to_dev(*g);
    if (M != ep.g.Np) return RRT_E_INVALID;
  }
  if (drop_on) {
    ep.drop_thresh = dc.thresh;
    ep.drop_scale = dc.scale;
    ep.drop_seed = dc.seed(drop_seed, drop_layer);
  }
  LinearPlan pl{};
  if (plan_linear(operands, (int)M, N, K, ep, &pl) != hipSuccess)
    return unsupported("linear: the launcher of this operand kind refuses the combination (K % 32 / % 64, dropout outside exact "
                       "fp32 or with an activation, activation on split images)");
  hipStream_t st = (hipStream_t)stream;
  if (operands == RRT_LINEAR_OPS_16) return (int)launch_linear16(A, B, C, (int)M, N, K, ep, st);
  if (operands == RRT_LINEAR_OPS_SPLIT) return (int)launch_linear_split(A, B, C, (int)M, N, K, ep, st);
  return (int)launch_linear((const float*)A, (const float*)B, C, (int)M, N, K, ep, st);
}

// ---- stage entries of the training backward's element-wise kernels (ln_bwd.hip) and the batched transpose (linear_bwd.hip):
//      one launcher each, arguments checked, the dropout words derived as the training entries derive them
//      (tests/test_train_blocks_matrix.py, test_train_blocks_grid_cpu.py)
namespace {
int check_act_stage(const void* a, const void* b, int64_t n, int32_t act, float drop_p, int32_t drop_layer, DropCfg* dc) {
  if (!a || !b || n <= 0 || n > (int64_t)1 << 40 || drop_layer < 0) return RRT_E_INVALID;
  if (make_drop(drop_p, dc)) return RRT_E_INVALID;
  if (act != RRT_ACT_GELU && act != RRT_ACT_RELU) return unsupported("activation pass: RRT_ACT_GELU or RRT_ACT_RELU");
  if (n % 4) return unsupported("activation pass: n must be a multiple of 4");
  return RRT_OK;
}
}  // namespace

int rrt_debug_act_forward_f32(const float* hpre, float* h, int64_t n, int32_t act, float drop_p, uint64_t drop_seed,
                              int32_t drop_layer, void* stream) {
  DropCfg dc{};
  const int rc = check_act_stage(hpre, h, n, act, drop_p, drop_layer, &dc);
  if (rc) return rc;
  return (int)launch_act_forward(hpre, h, (size_t)n, act, dc.thresh, dc.seed(drop_seed, drop_layer), dc.scale, (hipStream_t)stream);
}

int rrt_debug_act_backward_f32(float* dh, const float* hpre, int64_t n, int32_t act, float drop_p, uint64_t drop_seed,
                               int32_t drop_layer, void* stream) {
  DropCfg dc{};
  const int rc = check_act_stage(dh, hpre, n, act, drop_p, drop_layer, &dc);
  if (rc) return rc;
  if ((const float*)dh == hpre) return RRT_E_INVALID;
  return (int)launch_act_backward(dh, hpre, (size_t)n, act, dc.thresh, dc.seed(drop_seed, drop_layer), dc.scale, (hipStream_t)stream);
}

int rrt_debug_partition_rows_f32(const float* src, float* dst, int32_t dim, const rrt_grid* g, float drop_p, uint64_t drop_seed,
                                 int32_t drop_layer, float scale, void* stream) {
  if (!src || !dst || src == dst || !g || dim <= 0 || drop_layer < 0 || !(scale >= 0.f)) return RRT_E_INVALID;
  if (g->L <= 0 || g->H <= 0 || g->s <= 0 || g->regions_side <= 0 || (int64_t)g->regions_side * g->s != g->H ||
      g->L > (int64_t)g->H * g->H || (int64_t)g->H * g->H > (int64_t)1 << 24)
    return RRT_E_INVALID;
  DropCfg dc{};
  if (make_drop(drop_p, &dc)) return RRT_E_INVALID;
  if (dim % 4) return unsupported("partition rows: dim must be a multiple of 4");
  return (int)launch_partition_rows(src, dst, dim, to_dev(*g), dc.thresh, dc.seed(drop_seed, drop_layer), dc.scale * scale,
                                    (hipStream_t)stream);
}

int rrt_debug_drop_mask_f32(const float* src, float* dst, int64_t n, float drop_p, uint64_t drop_seed, int32_t drop_layer,
                            float scale, void* stream) {
  if (!src || !dst || n <= 0 || n > 0x7FFFFFFF || drop_layer < 0 || !(scale >= 0.f)) return RRT_E_INVALID;
  DropCfg dc{};
  if (make_drop(drop_p, &dc)) return RRT_E_INVALID;
  const unsigned seed = dc.seed(drop_seed, drop_layer);
  if (src == dst) return (int)launch_apply_drop_mask(dst, (int)n, 1, dc.thresh, seed, dc.scale * scale, (hipStream_t)stream);
  return (int)launch_copy_drop_mask(src, dst, (size_t)n, dc.thresh, seed, dc.scale * scale, (hipStream_t)stream);
}

int rrt_debug_transpose_batch_f32(const float* const* in, float* const* out, const int32_t* R, const int32_t* C, int32_t n_jobs,
                                  void* stream) {
  if (!in || !out || !R || !C || n_jobs <= 0) return RRT_E_INVALID;
  if (n_jobs > TRANSPOSE_MAX_JOBS) return unsupported("transpose batch: more jobs than one launch takes (2 * RRT_MAX_RMSA_LAYERS + 2)");
  TransposeJobs tj{};
  int64_t blocks = 0;
  for (int j = 0; j < n_jobs; ++j) {
    if (!in[j] || !out[j] || in[j] == out[j] || R[j] <= 0 || C[j] <= 0 || (int64_t)R[j] * C[j] > (int64_t)1 << 28) return RRT_E_INVALID;
    blocks += (int64_t)((R[j] + 31) / 32) * ((C[j] + 31) / 32);
    tj.in[j] = in[j];
    tj.out[j] = out[j];
    tj.R[j] = R[j];
    tj.C[j] = C[j];
  }
  if (blocks > 0x7FFFFFFF) return RRT_E_INVALID;
  tj.n = n_jobs;
  return (int)launch_transpose_batch(tj, (hipStream_t)stream);
}

}  // extern "C"

namespace {
// rrt_encoder_forward_train_f32; shortcut (rrt_encoder_tail_forward_train_f32): what all_shortcut adds, when it is not this
// call's x
int encoder_forward_train(const rrt_encoder_desc* desc, const rrt_encoder_weights* w, const float* x, const float* shortcut,
                          float* y, int64_t n_tokens, void* stash, size_t stash_bytes, float drop_p, uint64_t drop_seed,
                          const float* branch_scale, void* stream) {
  if (!desc || !w || !x || !y || x == y) return RRT_E_INVALID;
  DropCfg dc{};
  if (make_drop(drop_p, &dc)) return RRT_E_INVALID;
  Branch br{};
  if (make_branch(branch_scale, &br)) return RRT_E_INVALID;
  rrt_grid g{}, g8{};
  int rc = check_train(desc, n_tokens, &g, &g8);
  if (rc) return rc;
  Stash s = carve_stash(*desc, n_tokens, g, g8, nullptr);
  if (!stash || stash_bytes < s.bytes) return RRT_E_WORKSPACE;
  s = carve_stash(*desc, n_tokens, g, g8, (char*)stash);
  hipStream_t st = (hipStream_t)stream;
  const int D = desc->dim;
  const int64_t N = n_tokens;
  // TransLayer's FFN (ffn = 1): xf = xi + fc2(act(fc1(LN2(xi)))), stashing LN2's output and the pre-activation
  const GridDev gid = identity_grid(N);
  auto train_ffn = [&](const rrt_attn_weights& lw, const float* xi, int idx) -> int {
    if (!lw.norm2_w || !lw.norm2_b || !lw.fc1_w || !lw.fc1_b || !lw.fc2_w || !lw.fc2_b) return RRT_E_INVALID;
    RRT_TRY(launch_layernorm(xi, nullptr, lw.norm2_w, lw.norm2_b, s.ffn_u[idx], (int)N, D, st));
    LinearEpilogue e1{};
    e1.prec = desc->compute;
    e1.bias = lw.fc1_b;
    RRT_TRY(launch_linear(s.ffn_u[idx], lw.fc1_w, s.ffn_hpre[idx], (int)N, desc->ffn_hidden, D, e1, st));
    // the Mlp's two dropouts (rrt.py:38-40): after the activation and after fc2 (before the residual)
    RRT_TRY(launch_act_forward(s.ffn_hpre[idx], s.hscr, (size_t)N * desc->ffn_hidden, desc->ffn_act, dc.thresh,
                               dc.seed(drop_seed, 200 + 2 * idx), dc.scale, st));
    LinearEpilogue e2 = proj_epilogue(lw.fc2_b, xi, gid, RRT_COMPUTE_F32);      // (fc2 of the training FFN: exact fp32 in every mode)
    const float bsf = br.ffn[idx < RRT_MAX_RMSA_LAYERS ? idx : desc->n_rmsa_layers];
    e2.drop_thresh = dc.thresh;
    e2.drop_scale = dc.scale * bsf;
    e2.drop_on = dc.thresh || bsf != 1.0f;
    e2.drop_seed = dc.seed(drop_seed, 201 + 2 * idx);
    return (int)launch_linear(s.hscr, lw.fc2_w, s.xf[idx], (int)N, D, desc->ffn_hidden, e2, st);
  };
  const float* xin = x;
  const bool pos_first = desc->pos && desc->pos_pos == -1, pos_mid = desc->pos && desc->pos_pos == 0;
  if (desc->pos && (!w->pos_w[0] || (desc->pos == RRT_POS_PPEG && (!w->pos_w[1] || !w->pos_w[2])))) return RRT_E_INVALID;
  if (pos_first) {
    RRT_TRY(launch_peg(xin, w->pos_w, w->pos_b, s.xp, (int)N, D, desc->peg_k, desc->peg_1d, desc->pos == RRT_POS_PPEG, st));
    xin = s.xp;
  }
  for (int li = 0; li < desc->n_rmsa_layers; ++li) {
    if (pos_mid && li == 1) {
      RRT_TRY(launch_peg(xin, w->pos_w, w->pos_b, s.xp, (int)N, D, desc->peg_k, desc->peg_1d, desc->pos == RRT_POS_PPEG, st));
      xin = s.xp;
    }
    const rrt_attn_weights& lw = w->rmsa[li];
    if (!lw.norm_w || !lw.norm_b || !lw.qkv_w || !lw.proj_w || !lw.proj_b) return RRT_E_INVALID;
    if (desc->epeg && !lw.pe_w) return RRT_E_INVALID;
    const GridDev gd = to_dev(g);
    RRT_TRY(launch_ln_partition(xin, lw.norm_w, lw.norm_b, s.u[li], D, gd, st));
    const LinearEpilogue ep = qkv_epilogue(lw.qkv_b, D, desc->n_heads, desc->compute);
    const bool e2d = desc->epeg && desc->epeg_2d && desc->epeg_type == RRT_EPEG_ATTN;
    const bool evalue = desc->epeg && desc->epeg_type != RRT_EPEG_ATTN;
    // the inference path's fused kernel (projection + EPEG + attention per (region, head)) with the q | k | v tiles
    // also written to the stash, where the bag's regions fit it; else projection to the stash + attention from it
    const int ekf = desc->epeg ? desc->epeg_k : 0;
    const bool fused = !e2d && !evalue && desc->compute == RRT_COMPUTE_F32 &&
                       rmsa_fused_supported(gd.P, D, desc->n_heads, ekf) && rmsa_fused_supported_rows(gd.Np, D);
    if (fused) {
      RRT_TRY(launch_rmsa_fused(s.u[li], lw.qkv_w, lw.qkv_b, desc->epeg ? lw.pe_w : nullptr, s.o[li], gd.rs * gd.rs, gd.P, D,
                                desc->n_heads, ekf, RRT_COMPUTE_F32, st, s.qkv[li]));
    } else {
    RRT_TRY(launch_linear(s.u[li], lw.qkv_w, s.qkv[li], gd.Np, 3 * D, D, ep, st));
    if (e2d) {                                            // rmsa.py:78-79,106-108
      RRT_TRY(launch_attn_scoremap(s.qkv[li], lw.pe_w, s.o[li], s.smap, gd.rs * gd.rs, gd.P, D, desc->n_heads, desc->epeg_k, st));
    } else if (evalue) {                                  // rmsa.py:80-85,114-129; the stash keeps pe, v' = v + pe ('bf') and o + pe ('af')
      RRT_TRY(launch_value_pe(s.qkv[li], lw.pe_w, lw.pe_b, s.pe[li], gd.rs * gd.rs, gd.P, gd.s, D, desc->n_heads, desc->epeg_k,
                              desc->epeg_2d, st));
      if (desc->epeg_type == RRT_EPEG_VALUE_BF) RRT_TRY(launch_add_cols(s.qkv[li] + 2 * D, s.pe[li], (size_t)gd.Np, D, 3 * D, st));
      RRT_TRY(launch_region_attention(s.qkv[li], nullptr, s.o[li], gd.rs * gd.rs, gd.P, D, desc->n_heads, 0, st));
      if (desc->epeg_type == RRT_EPEG_VALUE_AF) RRT_TRY(launch_add_cols(s.o[li], s.pe[li], (size_t)gd.Np, D, D, st));
    } else
    RRT_TRY(launch_region_attention(s.qkv[li], desc->epeg ? lw.pe_w : nullptr, s.o[li], gd.rs * gd.rs, gd.P, D,
                                    desc->n_heads, desc->epeg ? desc->epeg_k : 0, st));
    }
    const bool drop_on = dc.thresh || br.attn[li] != 1.0f;
    LinearEpilogue ep2 = proj_epilogue(lw.proj_b, xin, gd, drop_on ? RRT_COMPUTE_F32 : desc->compute);      // the dropout epilogue exists in fp32 only
    ep2.drop_thresh = dc.thresh;
    ep2.drop_scale = dc.scale * br.attn[li];
    ep2.drop_on = drop_on;
    ep2.drop_seed = dc.seed(drop_seed, li);
    RRT_TRY(launch_linear(s.o[li], lw.proj_w, s.xout[li], gd.Np, D, D, ep2, st));
    xin = s.xout[li];
    if (desc->ffn) {
      rc = train_ffn(lw, xin, li);
      if (rc) return rc;
      xin = s.xf[li];
    }
  }
  const float* x0 = desc->all_shortcut ? (shortcut ? shortcut : x) : nullptr;
  if (!w->norm_w || !w->norm_b) return RRT_E_INVALID;
  if (desc->cr_msa) {
    const rrt_attn_weights& cw = w->crmsa;
    if (!cw.norm_w || !cw.norm_b || !cw.qkv_w || !cw.proj_w || !cw.proj_b) return RRT_E_INVALID;
    if (desc->crmsa_mlp ? (!w->phi0_w || !w->phi2_w) : !w->phi) return RRT_E_INVALID;
    const GridDev gd8 = to_dev(g8);
    const int k = desc->crmsa_k, R8 = gd8.rs * gd8.rs;
    if (desc->crmsa_mlp) {
      // the LayerNorm statistics the backward needs come out of the logits kernel (run on the first D*k floats of
      // W1 as a stand-in phi; its logits are overwritten by the MLP's two lines below)
      RRT_TRY(launch_crmsa_logits(xin, cw.norm_w, cw.norm_b, w->phi0_w, s.mean_rstd, s.logits, D, k, gd8, st));
      RRT_TRY(launch_ln_partition(xin, cw.norm_w, cw.norm_b, s.v8, D, gd8, st));
      LinearEpilogue e0{};
      e0.prec = desc->compute;
      RRT_TRY(launch_linear(s.v8, w->phi0_w, s.hid, gd8.Np, D / 4, D, e0, st));
      RRT_TRY(launch_crmsa_mlp_logits(s.hid, w->phi2_w, s.logits, gd8.Np, D / 4, k, st));
      RRT_TRY(launch_crmsa_combine(s.v8, nullptr, nullptr, nullptr, s.logits, s.wdisp, s.rep, nullptr, 0, D, k, gd8, st));
    } else {
      RRT_TRY(launch_crmsa_logits(xin, cw.norm_w, cw.norm_b, w->phi, s.mean_rstd, s.logits, D, k, gd8, st));
      RRT_TRY(launch_crmsa_combine(xin, cw.norm_w, cw.norm_b, s.mean_rstd, s.logits, s.wdisp, s.rep, nullptr, 0, D, k, gd8, st));
    }
    LinearEpilogue ep = qkv_epilogue(cw.qkv_b, D, desc->crmsa_heads, desc->compute);
    ep.solo = true;
    RRT_TRY(launch_linear(s.rep, cw.qkv_w, s.rep_qkv, k * R8, 3 * D, D, ep, st));
    RRT_TRY(launch_region_attention(s.rep_qkv, nullptr, s.rep_o, k, R8, D, desc->crmsa_heads, 0, st));
    LinearEpilogue ep2{};
    ep2.bias = cw.proj_b;
    // CR-MSA's branch is linear in rep2 (dispatch = sum_n wdisp * rep2): its stochastic-depth multiplier rides here
    const float bsc = br.attn[desc->n_rmsa_layers];
    ep2.drop_thresh = dc.thresh;
    ep2.drop_scale = dc.scale * bsc;
    ep2.drop_on = dc.thresh || bsc != 1.0f;
    ep2.drop_seed = dc.seed(drop_seed, DROP_LAYER_CRMSA);
    ep2.prec = ep2.drop_on ? RRT_COMPUTE_F32 : desc->compute;
    ep2.solo = true;                            // (as the qkv product above: K split inside the block, dropout epilogue included)
    RRT_TRY(launch_linear(s.rep_o, cw.proj_w, s.rep2, k * R8, D, D, ep2, st));
    if (desc->ffn) {
      // CR-MSA's TransLayer: x1 + dispatch -> xcr, FFN -> xf, then the shortcut, then the final LayerNorm
      RRT_TRY(launch_crmsa_dispatch_ln(xin, nullptr, s.wdisp, s.rep2, nullptr, nullptr, s.xcr, D, k, gd8, st));
      rc = train_ffn(cw, s.xcr, RRT_MAX_RMSA_LAYERS);
      if (rc) return rc;
      RRT_TRY(launch_layernorm(s.xf[RRT_MAX_RMSA_LAYERS], x0, nullptr, nullptr, s.x2, (int)N, D, st));
    } else {
      RRT_TRY(launch_crmsa_dispatch_ln(xin, x0, s.wdisp, s.rep2, nullptr, nullptr, s.x2, D, k, gd8, st));  // x2, no LN
    }
  } else {
    RRT_TRY(launch_layernorm(xin, x0, nullptr, nullptr, s.x2, (int)N, D, st));                            // x2 = x1 (+ x)
  }
  RRT_TRY(launch_layernorm(s.x2, nullptr, w->norm_w, w->norm_b, y, (int)N, D, st));
  return RRT_OK;
}

// rrt_encoder_backward_f32; d_shortcut (rrt_encoder_tail_backward_f32, all_shortcut = 1): the shortcut's gradient goes there
// instead of into dx
int encoder_backward(const rrt_encoder_desc* desc, const rrt_encoder_weights* w, const float* x, const float* dy,
                     const void* stash, size_t stash_bytes, const rrt_encoder_grads* gr, float* dx, float* d_shortcut,
                     int64_t n_tokens, void* workspace, size_t workspace_bytes, float drop_p, uint64_t drop_seed,
                     const float* branch_scale, void* stream) {
  if (!desc || !w || !x || !dy || !gr) return RRT_E_INVALID;
  DropCfg dc{};
  if (make_drop(drop_p, &dc)) return RRT_E_INVALID;
  Branch br{};
  if (make_branch(branch_scale, &br)) return RRT_E_INVALID;
  rrt_grid g{}, g8{};
  int rc = check_train(desc, n_tokens, &g, &g8);
  if (rc) return rc;
  Stash s = carve_stash(*desc, n_tokens, g, g8, nullptr);
  if (!stash || stash_bytes < s.bytes) return RRT_E_WORKSPACE;
  s = carve_stash(*desc, n_tokens, g, g8, (char*)stash);
  BwdWs b = carve_bwd(*desc, n_tokens, g, g8, nullptr);
  if (!workspace || workspace_bytes < b.bytes) return RRT_E_WORKSPACE;
  b = carve_bwd(*desc, n_tokens, g, g8, (char*)workspace);
  hipStream_t st = (hipStream_t)stream;
  const int D = desc->dim, L = desc->n_rmsa_layers;
  const int N = (int)n_tokens;
  if (!gr->norm) return RRT_E_INVALID;
  {
    // W^T of every attention Linear, for the dX products (dX = dY . W as the forward GEMM on W^T): one launch up front
    TransposeJobs tj{};
    // (a NULL weight or a full table used to drop the job silently: the dX product then read an unwritten W^T image)
    bool tj_bad = false;
    auto add = [&](const float* wsrc, float* wt, int n_out, int k_in) {
      if (!wsrc || !wt || tj.n >= TRANSPOSE_MAX_JOBS) { tj_bad = true; return; }
      tj.in[tj.n] = wsrc; tj.out[tj.n] = wt; tj.R[tj.n] = n_out; tj.C[tj.n] = k_in;
      ++tj.n;
    };
    for (int li = 0; li < desc->n_rmsa_layers; ++li) {
      add(w->rmsa[li].qkv_w, b.wt_qkv[li], 3 * D, D);
      add(w->rmsa[li].proj_w, b.wt_proj[li], D, D);
    }
    if (desc->cr_msa) {
      add(w->crmsa.qkv_w, b.wt_cr_qkv, 3 * D, D);
      add(w->crmsa.proj_w, b.wt_cr_proj, D, D);
    }
    if (tj_bad) return RRT_E_INVALID;
    RRT_TRY(launch_transpose_batch(tj, st));
  }
  // Parameter-gradient sums that nothing downstream reads leave the dependent chain: the stages below append their reduce
  // jobs here and one launch at the end of the pass runs them all (round 6: four 5-9 us launches -> one).  Each stage
  // therefore gets partial buffers of its own (ln_part(), tappart[li], dxpart).
  ReduceJobs rj{};
  static const bool no_defer = rrt_tune_env("RRT_NO_DEFER_REDUCE") != nullptr;      // (A/B, tuning build only)
  ReduceJobs* const defer = no_defer ? nullptr : &rj;
  int ln_calls = 0;
  auto ln_part = [&]() { return b.lnpart + (size_t)(ln_calls++) * b.lnpart_stride; };
  // final LayerNorm
  RRT_TRY(launch_ln_backward(dy, s.x2, w->norm_w, nullptr, b.dx2, gr->norm, ln_part(), N, D, nullptr, st, defer));
  const float* cur = b.dx2;   // gradient w.r.t. the activations entering the stage being undone
  // FFN backward (ffn = 1): given d xf in `cur`, the gradient w.r.t. the FFN's input xi goes to the other
  // ping-pong buffer; fc2 / fc1 through the linear backward, the activation through its own pass, LN2 last
  auto ffn_backward = [&](const rrt_attn_weights& lw, const rrt_attn_grads& lg, const float* xi, int idx) -> int {
    if (!lg.norm2 || !lg.fc1_w || !lg.fc1_b || !lg.fc2_w || !lg.fc2_b) return RRT_E_INVALID;
    const int Hd = desc->ffn_hidden;
    RRT_TRY(launch_act_forward(s.ffn_hpre[idx], b.fh, (size_t)N * Hd, desc->ffn_act, dc.thresh, dc.seed(drop_seed, 200 + 2 * idx),
                               dc.scale, st));
    const float* dyf = cur;                        // d(fc2 output): the residual's gradient through the second mask
    const float bsf = br.ffn[idx < RRT_MAX_RMSA_LAYERS ? idx : desc->n_rmsa_layers];
    if (dc.thresh || bsf != 1.0f) {
      RRT_TRY(launch_copy_drop_mask(cur, b.fdu, (size_t)N * D, dc.thresh, dc.seed(drop_seed, 201 + 2 * idx), dc.scale * bsf, st));
      dyf = b.fdu;
    }
    RRT_TRY(launch_linear_backward(dyf, b.fh, lw.fc2_w, b.fdh, lg.fc2_w, lg.fc2_b, N, D, Hd, desc->compute, b.lin, st));
    RRT_TRY(launch_act_backward(b.fdh, s.ffn_hpre[idx], (size_t)N * Hd, desc->ffn_act, dc.thresh, dc.seed(drop_seed, 200 + 2 * idx),
                                dc.scale, st));
    RRT_TRY(launch_linear_backward(b.fdh, s.ffn_u[idx], lw.fc1_w, b.fdu, lg.fc1_w, lg.fc1_b, N, Hd, D, desc->compute, b.lin, st));
    float* nxt = (cur == b.dxa) ? b.dxb : b.dxa;
    RRT_TRY(launch_ln_backward(b.fdu, xi, lw.norm2_w, cur, nxt, lg.norm2, ln_part(), N, D, nullptr, st, defer));
    cur = nxt;
    return RRT_OK;
  };
  // PEG / PPEG backward: d(stage output) in `cur` -> d(stage input) in the other buffer, plus the convs' gradients
  auto peg_backward = [&](const float* xstage_in) -> int {
    const bool ppeg = desc->pos == RRT_POS_PPEG;
    for (int i = 0; i < (ppeg ? 3 : 1); ++i)
      if (!gr->pos_w[i] || (w->pos_b[i] && !gr->pos_b[i])) return RRT_E_INVALID;
    float* nxt = (cur == b.dxa) ? b.dxb : b.dxa;
    float* dbp[3] = {w->pos_b[0] ? gr->pos_b[0] : nullptr, w->pos_b[1] ? gr->pos_b[1] : nullptr,
                     w->pos_b[2] ? gr->pos_b[2] : nullptr};
    RRT_TRY(launch_peg_backward(xstage_in, cur, w->pos_w, nxt, gr->pos_w, dbp, N, D, desc->peg_k, desc->peg_1d, ppeg, b.pegws, st));
    cur = nxt;
    return RRT_OK;
  };
  if (desc->cr_msa && desc->ffn) {
    rc = ffn_backward(w->crmsa, gr->crmsa, s.xcr, RRT_MAX_RMSA_LAYERS);
    if (rc) return rc;
  }
  if (desc->cr_msa) {
    const rrt_attn_weights& cw = w->crmsa;
    const rrt_attn_grads& cg = gr->crmsa;
    if (!cg.norm || !cg.qkv_w || !cg.proj_w || !cg.proj_b || (cw.qkv_b && !cg.qkv_b)) return RRT_E_INVALID;
    if (desc->crmsa_mlp ? (!gr->phi0_w || !gr->phi2_w) : !gr->phi) return RRT_E_INVALID;
    const GridDev gd8 = to_dev(g8);
    const int k = desc->crmsa_k, R8 = gd8.rs * gd8.rs;
    const float* x1 = L > 0 ? (desc->ffn ? s.xf[L - 1] : s.xout[L - 1]) : (desc->pos && desc->pos_pos == -1 ? s.xp : x);
    const float* up = cur;                                   // d x2 (after the FFN backward when ffn = 1)
    float* dx1 = (cur == b.dxa) ? b.dxb : b.dxa;
    RRT_TRY(launch_crmsa_tokdot(up, nullptr, nullptr, nullptr, s.rep2, b.dWd, D, k, gd8, st));
    RRT_TRY(launch_crmsa_wsum(up, s.wdisp, b.d_rep2, D, k, gd8, st));
    RRT_TRY(launch_apply_drop_mask(b.d_rep2, k * R8, D, dc.thresh, dc.seed(drop_seed, DROP_LAYER_CRMSA),
                                   dc.scale * br.attn[L], st));
    RRT_TRY(launch_linear_backward(b.d_rep2, s.rep_o, cw.proj_w, b.d_rep_o, cg.proj_w, cg.proj_b, k * R8, D, D, desc->compute,
                                   b.lin, st, b.wt_cr_proj));
    RRT_TRY(launch_attention_backward(s.rep_qkv, nullptr, s.rep_o, b.d_rep_o, b.d_rep_qkv, nullptr, b.attnpart_cr, k,
                                      R8, D, desc->crmsa_heads, 0, st));
    RRT_TRY(launch_linear_backward(b.d_rep_qkv, s.rep, cw.qkv_w, b.d_rep, cg.qkv_w, cg.qkv_b, k * R8, 3 * D, D, desc->compute,
                                   b.lin, st, b.wt_cr_qkv));
    RRT_TRY(launch_crmsa_tokdot(x1, s.mean_rstd, cw.norm_w, cw.norm_b, b.d_rep, b.dC, D, k, gd8, st));
    RRT_TRY(launch_crmsa_bwd_region(s.logits, b.dC, b.dWd, b.dlg, b.Cw, k, gd8, st));
    if (desc->crmsa_mlp) {
      // phi = Linear(D, D/4) -> Tanh -> Linear(D/4, k) (rmsa.py:248-252): d hid, then the two weight gradients as
      // TN products over the Np8 slots and the logits' path into v as a GEMM row block (pad slots carry v = 0 and
      // tanh(0) = 0, so they add nothing to dW1 / dW2)
      const int hdim = D / 4;
      RRT_TRY(launch_crmsa_mlp_bwd_hidden(s.hid, b.dlg, w->phi2_w, b.th, b.dhid, (size_t)gd8.Np, hdim, k, st));
      RRT_TRY(launch_gemm_tn(b.dlg, b.th, gr->phi2_w, b.tnscratch, gd8.Np, k, hdim, st));          // dW2 [k, D/4]
      RRT_TRY(launch_gemm_tn(b.dhid, s.v8, gr->phi0_w, b.tnscratch, gd8.Np, hdim, D, st));         // dW1 [D/4, D]
      if (hdim % 32 == 0) {
        RRT_TRY(launch_transpose(w->phi0_w, b.w1t, hdim, D, st));                                  // W1^T [D, D/4]
        LinearEpilogue ev{};
        ev.prec = desc->compute;
        RRT_TRY(launch_linear(b.dhid, b.w1t, b.dvphi, gd8.Np, D, hdim, ev, st));                   // d v_phi = d hid . W1
      } else {                                             // hidden width not a GEMM K tile (dim % 128 != 0)
        RRT_TRY(launch_small_k_matmul(b.dhid, w->phi0_w, b.dvphi, gd8.Np, D, hdim, st));
      }
      // (the reduce launch writes LayerNorm's gradients where they belong when the caller's buffer takes 16-byte stores: the
      //  4 KB copy -- and, below, the transpose of d phi -- were two 5 us launches of the dependent chain)
      const bool direct = ((uintptr_t)cg.norm & 15) == 0;
      RRT_TRY(launch_crmsa_bwd_dx(x1, up, s.mean_rstd, cw.norm_w, cw.norm_b, b.dvphi, b.Cw, b.dlg, b.d_rep, dx1,
                                  direct ? cg.norm : b.rows, b.dxpart, D, k, gd8, true, st, nullptr, direct ? defer : nullptr));
      if (!direct) RRT_TRY(hipMemcpyAsync(cg.norm, b.rows, (size_t)2 * D * sizeof(float), hipMemcpyDeviceToDevice, st));
    } else if (((uintptr_t)cg.norm & 15) == 0) {
      RRT_TRY(launch_crmsa_bwd_dx(x1, up, s.mean_rstd, cw.norm_w, cw.norm_b, w->phi, b.Cw, b.dlg, b.d_rep, dx1,
                                  cg.norm, b.dxpart, D, k, gd8, false, st, gr->phi, defer));
    } else {
      RRT_TRY(launch_crmsa_bwd_dx(x1, up, s.mean_rstd, cw.norm_w, cw.norm_b, w->phi, b.Cw, b.dlg, b.d_rep, dx1,
                                  b.rows, b.dxpart, D, k, gd8, false, st));
      RRT_TRY(hipMemcpyAsync(cg.norm, b.rows, (size_t)2 * D * sizeof(float), hipMemcpyDeviceToDevice, st));
      RRT_TRY(launch_transpose(b.rows + 2 * (size_t)D, gr->phi, k, D, st));      // [k, D] -> phi's [D, k]
    }
    cur = dx1;
  }
  for (int li = L - 1; li >= 0; --li) {
    const rrt_attn_weights& lw = w->rmsa[li];
    const rrt_attn_grads& lg = gr->rmsa[li];
    if (!lg.norm || !lg.qkv_w || !lg.proj_w || !lg.proj_b || (lw.qkv_b && !lg.qkv_b) || (desc->epeg && !lg.pe_w))
      return RRT_E_INVALID;
    const GridDev gd = to_dev(g);
    const bool pos_in = desc->pos && ((desc->pos_pos == -1 && li == 0) || (desc->pos_pos == 0 && li == 1));
    const float* xprev = li > 0 ? (desc->ffn ? s.xf[li - 1] : s.xout[li - 1]) : x;   // before a PEG stage, if any
    const float* xin = pos_in ? s.xp : xprev;
    if (desc->ffn) {
      rc = ffn_backward(lw, lg, s.xout[li], li);
      if (rc) return rc;
    }
    RRT_TRY(launch_partition_rows(cur, b.dz, D, gd, dc.thresh, dc.seed(drop_seed, li), dc.scale * br.attn[li], st));
    RRT_TRY(launch_linear_backward(b.dz, s.o[li], lw.proj_w, b.dO, lg.proj_w, lg.proj_b, gd.Np, D, D, desc->compute, b.lin, st,
                                   b.wt_proj[li]));
    const bool e2d = desc->epeg && desc->epeg_2d && desc->epeg_type == RRT_EPEG_ATTN;
    const bool evalue = desc->epeg && desc->epeg_type != RRT_EPEG_ATTN;
    if (e2d) {
      RRT_TRY(launch_attn_scoremap_backward(s.qkv[li], lw.pe_w, b.dO, b.dqkv, lg.pe_w, b.smap, gd.rs * gd.rs, gd.P, D,
                                            desc->n_heads, desc->epeg_k, st));
    } else if (evalue) {
      if (lw.pe_b && !lg.pe_b) return RRT_E_INVALID;
      const int nreg = gd.rs * gd.rs;
      if (desc->epeg_type == RRT_EPEG_VALUE_BF) {
        // attention ran on v' = v + pe: its backward gives dv' (v columns of dqkv) = d pe; the conv read v = v' - pe
        RRT_TRY(launch_attention_backward(s.qkv[li], nullptr, s.o[li], b.dO, b.dqkv, nullptr, b.attnpart, nreg, gd.P, D,
                                          desc->n_heads, 0, st));
        RRT_TRY(launch_copy_cols(b.dpe, b.dqkv, (size_t)gd.Np, D, 3 * D, 2 * D, st));
        RRT_TRY(launch_value_pe_backward(b.dpe, s.qkv[li], s.pe[li], lw.pe_w, b.dqkv, lg.pe_w, lw.pe_b ? lg.pe_b : nullptr, nreg,
                                         gd.P, gd.s, D, desc->n_heads, desc->epeg_k, desc->epeg_2d, st));
      } else {
        // proj read o + pe: d pe = dO; the attention's own output is (o + pe) - pe (into dz, dead since the proj backward)
        RRT_TRY(launch_sub(b.dz, s.o[li], s.pe[li], (size_t)gd.Np * D, st));
        RRT_TRY(launch_attention_backward(s.qkv[li], nullptr, b.dz, b.dO, b.dqkv, nullptr, b.attnpart, nreg, gd.P, D,
                                          desc->n_heads, 0, st));
        RRT_TRY(launch_value_pe_backward(b.dO, s.qkv[li], nullptr, lw.pe_w, b.dqkv, lg.pe_w, lw.pe_b ? lg.pe_b : nullptr, nreg,
                                         gd.P, gd.s, D, desc->n_heads, desc->epeg_k, desc->epeg_2d, st));
      }
    } else
    RRT_TRY(launch_attention_backward(s.qkv[li], desc->epeg ? lw.pe_w : nullptr, s.o[li], b.dO, b.dqkv,
                                      desc->epeg ? lg.pe_w : nullptr, b.attnpart, gd.rs * gd.rs, gd.P, D,
                                      desc->n_heads, desc->epeg ? desc->epeg_k : 0, st, defer, b.tappart[li]));
    RRT_TRY(launch_linear_backward(b.dqkv, s.u[li], lw.qkv_w, b.dz, lg.qkv_w, lg.qkv_b, gd.Np, 3 * D, D, desc->compute, b.lin,
                                   st, b.wt_qkv[li]));                         // dU -> dz (dead)
    float* nxt = (cur == b.dxa) ? b.dxb : b.dxa;
    RRT_TRY(launch_ln_backward(b.dz, xin, lw.norm_w, cur, nxt, lg.norm, ln_part(), N, D, &gd, st, defer));
    cur = nxt;
    if (pos_in) {
      rc = peg_backward(xprev);
      if (rc) return rc;
    }
  }
  if (desc->pos && desc->pos_pos == -1 && L == 0) {       // no R-MSA layer: the PEG stage feeds CR-MSA directly
    rc = peg_backward(x);
    if (rc) return rc;
  }
  if (dx) RRT_TRY(launch_layernorm(cur, desc->all_shortcut && !d_shortcut ? b.dx2 : nullptr, nullptr, nullptr, dx, N, D, st));
  if (desc->all_shortcut && d_shortcut)
    RRT_TRY(hipMemcpyAsync(d_shortcut, b.dx2, (size_t)N * D * sizeof(float), hipMemcpyDeviceToDevice, st));
  RRT_TRY(launch_reduce_jobs(rj, st));
  return RRT_OK;
}

// the tail entries take what encoder_tail takes: no attention layer and no PEG stage in front of CR-MSA
int check_tail_desc(const rrt_encoder_desc* desc) {
  if (!desc) return RRT_E_INVALID;
  if (desc->n_rmsa_layers != 0 || desc->pos != RRT_POS_NONE)
    return unsupported("encoder_tail: n_rmsa_layers must be 0 and pos none (the part behind the attention layers)");
  return RRT_OK;
}
}  // namespace

extern "C" {

int rrt_encoder_forward_train_f32(const rrt_encoder_desc* desc, const rrt_encoder_weights* w, const float* x,
                                  float* y, int64_t n_tokens, void* stash, size_t stash_bytes, float drop_p,
                                  uint64_t drop_seed, const float* branch_scale, void* stream) {
  return encoder_forward_train(desc, w, x, nullptr, y, n_tokens, stash, stash_bytes, drop_p, drop_seed, branch_scale, stream);
}

int rrt_encoder_backward_f32(const rrt_encoder_desc* desc, const rrt_encoder_weights* w, const float* x,
                             const float* dy, const void* stash, size_t stash_bytes, const rrt_encoder_grads* gr,
                             float* dx, int64_t n_tokens, void* workspace, size_t workspace_bytes, float drop_p,
                             uint64_t drop_seed, const float* branch_scale, void* stream) {
  return encoder_backward(desc, w, x, dy, stash, stash_bytes, gr, dx, nullptr, n_tokens, workspace, workspace_bytes, drop_p,
                          drop_seed, branch_scale, stream);
}

int rrt_encoder_tail_forward_train_f32(const rrt_encoder_desc* desc, const rrt_encoder_weights* w, const float* x1,
                                       const float* x0, float* y, int64_t n_tokens, void* stash, size_t stash_bytes,
                                       float drop_p, uint64_t drop_seed, const float* branch_scale, void* stream) {
  int rc = check_tail_desc(desc);
  if (rc) return rc;
  if (desc->all_shortcut && !x0) return RRT_E_INVALID;
  return encoder_forward_train(desc, w, x1, x0, y, n_tokens, stash, stash_bytes, drop_p, drop_seed, branch_scale, stream);
}

int rrt_encoder_tail_backward_f32(const rrt_encoder_desc* desc, const rrt_encoder_weights* w, const float* x1, const float* dy,
                                  const void* stash, size_t stash_bytes, const rrt_encoder_grads* gr, float* d_x1, float* d_x0,
                                  int64_t n_tokens, void* workspace, size_t workspace_bytes, float drop_p, uint64_t drop_seed,
                                  const float* branch_scale, void* stream) {
  int rc = check_tail_desc(desc);
  if (rc) return rc;
  if (desc->all_shortcut && !d_x0) return RRT_E_INVALID;
  return encoder_backward(desc, w, x1, dy, stash, stash_bytes, gr, d_x1, d_x0, n_tokens, workspace, workspace_bytes, drop_p,
                          drop_seed, branch_scale, stream);
}

}  // extern "C"
