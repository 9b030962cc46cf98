// mil_pool.hip -- ABMIL attention pooling + predictor behind the encoder.
//
// Replaces modules/datten.py:28-38 (Attention.forward) / :69-83 (AttentionGated.forward) after their
// first Linear(+activation), and modules/rrt.py:241 (predictor):
//     a_n    = wc . h_n (+ bc)            h_n = hid_a[n]  or  hid_a[n] * hid_b[n] (gated)
//     A      = softmax_n(a)               over the N tokens of the bag
//     pooled = sum_n A_n y_n              [dim]
//     logits = pred_w pooled + pred_b     [n_classes]
// The softmax over N is an online softmax over POOL_CHUNK-token chunks: every block emits
// (m_b, l_b, v_b = sum exp(a_n - m_b) y_n), one merge block rescales and adds them (pool_core.h: the pieces every head's
// pooling kernels are built from; the kernels here are those pieces at one branch plus the predictor).  HBM-bound:
// reads y (N*dim) and the hidden rows (N*hid) once; the 18 MB of y never has to be re-read by a
// separate softmax / matmul pair, and nothing of size N x dim is written.
#include "pool_core.h"

namespace {

// part layout per chunk: [dim] weighted sum, then m, l (padded to dim + 4 floats)
__device__ __forceinline__ size_t part_stride(int dim) { return (size_t)dim + 4; }

__global__ __launch_bounds__(256) void pool_partial_kernel(const float* __restrict__ y,
                                                           const float* __restrict__ hid_a,
                                                           const float* __restrict__ hid_b,
                                                           const float* __restrict__ wc,
                                                           const float* __restrict__ bc,
                                                           float* __restrict__ a_raw,
                                                           float* __restrict__ part, int N, int dim, int hid) {
  __shared__ float s_a[POOL_CHUNK];
  __shared__ float s_e[1][POOL_CHUNK];
  extern __shared__ __attribute__((aligned(16))) char smem[];     // [dim/4 <= 128] float4: second row group's partial
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * POOL_CHUNK;
  const int cnt = min(POOL_CHUNK, N - n0);

  // ---- scores: one wave per token, POOL_CHUNK / 4 tokens per wave
  const float b = bc ? bc[0] : 0.f;
  for (int t = wave; t < cnt; t += 4) {
    float s[1];
    gate_scores_row<1>(hid_a, hid_b, wc, (size_t)(n0 + t) * hid, hid, lane, s);
    const float acc = s[0] + b;
    if (lane == 0) {
      s_a[t] = acc;
      a_raw[n0 + t] = acc;
    }
  }
  __syncthreads();
  // ---- chunk max / exp / sum (every thread redundantly: cnt <= 32 LDS reads)
  float m = -3.0e38f;
  for (int t = 0; t < cnt; ++t) m = fmaxf(m, s_a[t]);
  if (tid < POOL_CHUNK) s_e[0][tid] = tid < cnt ? __expf(s_a[tid] - m) : 0.f;
  __syncthreads();
  float l = 0.f;
  for (int t = 0; t < cnt; ++t) l += s_e[0][t];

  // ---- weighted sum of the chunk's rows
  float* out = part + (size_t)blockIdx.x * part_stride(dim);
  chunk_weighted_rowsum<1>(y, s_e, (float4(*)[128])smem, out, n0, cnt, dim);
  if (tid == 0) {
    out[dim] = m;
    out[dim + 1] = l;
  }
}

// One block: the merge core over the chunk partials, then the predictor and the attention row the reference returns
// (normalised, or raw scores for no_norm=True).
__global__ __launch_bounds__(1024) void pool_merge_kernel(const float* __restrict__ part,
                                                          const float* __restrict__ a_raw,
                                                          const float* __restrict__ pred_w,
                                                          const float* __restrict__ pred_b,
                                                          float* __restrict__ pooled,
                                                          float* __restrict__ logits, float* __restrict__ attn,
                                                          int no_norm, int N, int dim, int n_classes, int nb) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const PoolMerged p = pool_merge_core(part + dim, 1, part, part_stride(dim), nb, dim, smem, pooled);

  // predictor: one wave per class
  for (int j = wave; j < n_classes; j += 16) {
    const float acc = wave_row_dot(pred_w + (size_t)j * dim, p.s_pool, dim, lane);
    if (lane == 0) logits[j] = acc + (pred_b ? pred_b[j] : 0.f);
  }
  if (attn) {
    for (int n = tid; n < N; n += 1024) {
      const float a = a_raw[n];
      attn[n] = no_norm ? a : __expf(a - p.M) * p.invL;
    }
  }
}

// ---- backward of the pooling (training of the slide classifier; adjoint of datten.py:28-38 / :69-83 after the first Linear):
//     s_n = wc . h_n + bc ,  A = softmax_n(s) ,  pooled = sum_n A_n y_n         (h = hid_a, or hid_a * hid_b when gated)
// given d pooled [dim] (and optionally d A [N], d s [N] for callers that use the returned attention / raw scores):
//     dA_n = y_n . dpooled (+ dA_ext_n)      ds_n = A_n (dA_n - c) (+ ds_ext_n) ,  c = sum_m A_m dA_m = pooled . dpooled (+ c_ext)
//     dy_n = A_n dpooled      dh_n = ds_n wc      d wc = sum_n ds_n h_n      d bc = sum_n ds_n
// One wave per token, POOL_BWD_ROWS tokens per block; per-block partials of (d wc | d bc) -> launch_reduce_partials.
constexpr int POOL_BWD_ROWS = 32;
__global__ __launch_bounds__(256) void pool_backward_kernel(const float* __restrict__ y, const float* __restrict__ hid_a,
                                                            const float* __restrict__ hid_b, const float* __restrict__ wc,
                                                            const float* __restrict__ attn, const float* __restrict__ pooled,
                                                            const float* __restrict__ d_pooled, const float* __restrict__ d_attn,
                                                            const float* __restrict__ d_raw, const float* __restrict__ c_ext,
                                                            float* __restrict__ dy, float* __restrict__ dhid_a,
                                                            float* __restrict__ dhid_b, float* __restrict__ part, int N, int dim,
                                                            int hid) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* s_dp = (float*)smem;                        // d pooled [dim]
  float* s_acc = s_dp + dim;                         // [4 waves][hid + 4]: this block's d wc | d bc partial
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __shared__ float s_c[4];
  for (int c = tid; c < 4 * (hid + 4); c += 256) s_acc[c] = 0.f;
  pool_backward_stage(d_pooled, pooled, s_dp, s_c, dim);
  __syncthreads();
  const float cc = pool_backward_c(s_c) + (c_ext ? c_ext[0] : 0.f);
  float* myacc = s_acc + wave * (hid + 4);
  const int n0 = blockIdx.x * POOL_BWD_ROWS;
  float dbc = 0.f;
  for (int t = wave; t < POOL_BWD_ROWS; t += 4) {
    const int n = n0 + t;
    if (n >= N) break;
    const float a = attn[n];
    const float* yr = y + (size_t)n * dim;
    float da = 0.f;
    for (int c = lane * 4; c < dim; c += 256) {
      const float4 v = *(const float4*)(yr + c);
      const float4 d = *(const float4*)(s_dp + c);
      da += (v.x * d.x + v.y * d.y) + (v.z * d.z + v.w * d.w);
      *(float4*)(dy + (size_t)n * dim + c) = make_float4(a * d.x, a * d.y, a * d.z, a * d.w);
    }
    da = wave_sum(da) + (d_attn ? d_attn[n] : 0.f);
    const float ds = a * (da - cc) + (d_raw ? d_raw[n] : 0.f);
    dbc += ds;
    for (int c = lane * 4; c < hid; c += 256) {
      const float4 w = *(const float4*)(wc + c);
      float4 ha = *(const float4*)(hid_a + (size_t)n * hid + c);
      float4 g = make_float4(ds * w.x, ds * w.y, ds * w.z, ds * w.w);          // d (h_a h_b) (or d h_a)
      float4 h = ha;
      if (hid_b) {
        const float4 hb = *(const float4*)(hid_b + (size_t)n * hid + c);
        *(float4*)(dhid_b + (size_t)n * hid + c) = make_float4(g.x * ha.x, g.y * ha.y, g.z * ha.z, g.w * ha.w);
        h = make_float4(ha.x * hb.x, ha.y * hb.y, ha.z * hb.z, ha.w * hb.w);
        g = make_float4(g.x * hb.x, g.y * hb.y, g.z * hb.z, g.w * hb.w);
      }
      *(float4*)(dhid_a + (size_t)n * hid + c) = g;
      float4 acc = *(float4*)(myacc + c);
      acc.x += ds * h.x; acc.y += ds * h.y; acc.z += ds * h.z; acc.w += ds * h.w;
      *(float4*)(myacc + c) = acc;
    }
  }
  if (lane == 0) myacc[hid] = dbc;
  __syncthreads();
  float* out = part + (size_t)blockIdx.x * (hid + 4);
  for (int c = tid; c < hid + 1; c += 256)
    out[c] = (s_acc[c] + s_acc[(hid + 4) + c]) + (s_acc[2 * (hid + 4) + c] + s_acc[3 * (hid + 4) + c]);
}

}  // namespace

// The backward block stays inside the default LDS limit (no head builds a hidden width near it: 128 everywhere in the reference).
size_t pool_backward_lds_bytes(int dim, int hid) { return ((size_t)dim + 4 * ((size_t)hid + 4)) * sizeof(float); }
bool pool_merge_fits(int64_t N, int dim) {
  return pool_merge_lds_bytes((size_t)((N + POOL_CHUNK - 1) / POOL_CHUNK), dim) <= POOL_MERGE_LDS_MAX;
}
bool pool_backward_fits(int dim, int hid) { return pool_backward_lds_bytes(dim, hid) <= POOL_LDS_DEFAULT; }

// d wc [hid] and d bc [1] come out as dwcb [hid + 4] (d bc at [hid]); part: ceil(N / 32) * (hid + 4) floats
hipError_t launch_pool_backward(const float* y, const float* hid_a, const float* hid_b, const float* wc, const float* attn,
                                const float* pooled, const float* d_pooled, const float* d_attn, const float* d_raw,
                                const float* c_ext, float* dy, float* dhid_a, float* dhid_b, float* dwcb, float* part, int N,
                                int dim, int hid, hipStream_t st) {
  const int nb = (N + POOL_BWD_ROWS - 1) / POOL_BWD_ROWS;
  const size_t lds = pool_backward_lds_bytes(dim, hid);
  if (lds > POOL_LDS_DEFAULT) return hipErrorInvalidValue;      // (the C ABI refuses these shapes before it gets here)
  pool_backward_kernel<<<dim3(nb), dim3(256), lds, st>>>(y, hid_a, hid_b, wc, attn, pooled, d_pooled, d_attn, d_raw, c_ext, dy,
                                                         dhid_a, dhid_b, part, N, dim, hid);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_reduce_partials(part, dwcb, nb, (size_t)hid + 4, st);
}

size_t pool_backward_part_floats(int N, int hid) { return (size_t)((N + POOL_BWD_ROWS - 1) / POOL_BWD_ROWS) * (hid + 4); }

hipError_t launch_pool_partial(const float* y, const float* hid_a, const float* hid_b, const float* wc,
                               const float* bc, float* a_raw, float* part, int N, int dim, int hid,
                               hipStream_t st) {
  const int nb = (N + POOL_CHUNK - 1) / POOL_CHUNK;
  const size_t lds = (size_t)128 * sizeof(float4);
  pool_partial_kernel<<<dim3(nb), dim3(256), lds, st>>>(y, hid_a, hid_b, wc, bc, a_raw, part, N, dim, hid);
  return hipGetLastError();
}

hipError_t launch_pool_merge(const float* part, const float* a_raw, const float* pred_w, const float* pred_b,
                             float* pooled, float* logits, float* attn, int no_norm, int N, int dim,
                             int n_classes, hipStream_t st) {
  const int nb = (N + POOL_CHUNK - 1) / POOL_CHUNK;
  const size_t lds = pool_merge_lds_bytes(nb, dim);
  if (lds > POOL_MERGE_LDS_MAX) return hipErrorInvalidValue;    // (the C ABI refuses these shapes before it gets here)
  auto kern = pool_merge_kernel;
  pool_raise_lds_limit((const void*)kern, lds);
  kern<<<dim3(1), dim3(1024), lds, st>>>(part, a_raw, pred_w, pred_b, pooled, logits, attn, no_norm, N, dim,
                                         n_classes, nb);
  return hipGetLastError();
}
