// clam_pool.hip -- multi-branch gated attention pooling and top-k instance selection: the CLAM_SB / CLAM_MB heads
// (modules/clam.py:25-74 Attn_Net / Attn_Net_Gated after their first Linear + activation, :172-177, :203 / :293, and the
// two torch.topk calls of inst_eval / inst_eval_out :141-143, :161) behind the encoder.
//
//     s[c, n] = c_w[c] . h_n + c_b[c]        h_n = hid_a[n]  or  hid_a[n] * hid_b[n] (gated),  c = 0 .. K-1 branches
//     A[c, :] = softmax_n(s[c, :])           over the N tokens of the bag, per branch
//     M[c, :] = sum_n A[c, n] y_n            [K, dim]
//
// The online softmax of pool_core.h: every POOL_CHUNK-token block emits (m, l, sum e^{s-m} y) -- here for every
// branch -- and one merge block per branch rescales and adds them.  The point of the kernel is that a y row is read ONCE for
// all K branches: the K float4 accumulators of a column lane live in registers (K = 8: 32 VGPRs), so CLAM_MB's n_classes
// branches read y once, not n_classes times.  Nothing of size N x dim is written.  Every sum has a fixed order (no atomics): the
// same inputs give the same bits, whatever else is in flight.
#include "pool_core.h"

namespace {

// part layout per chunk: [K][dim] weighted sums, then m[K], l[K] (padded: K * dim + 16 floats)
__host__ __device__ __forceinline__ size_t bpart_stride(int K, int dim) { return (size_t)K * dim + 16; }

template <int K>
__global__ __launch_bounds__(256) void branch_partial_kernel(const float* __restrict__ y, const float* __restrict__ hid_a,
                                                             const float* __restrict__ hid_b, const float* __restrict__ wc,
                                                             const float* __restrict__ bc, float* __restrict__ a_raw,
                                                             float* __restrict__ part, int N, int dim, int hid) {
  __shared__ float s_a[K][POOL_CHUNK];
  __shared__ float s_e[K][POOL_CHUNK];
  __shared__ float s_m[K];
  __shared__ __attribute__((aligned(16))) float4 red[K][128];      // second row group's partials
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * POOL_CHUNK;
  const int cnt = min(POOL_CHUNK, N - n0);

  // ---- scores: one wave per token, the hidden row read once for the K score rows
  for (int t = wave; t < cnt; t += 4) {
    float s[K];
    gate_scores_row<K>(hid_a, hid_b, wc, (size_t)(n0 + t) * hid, hid, lane, s);
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] += bc ? bc[k] : 0.f;
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        s_a[k][t] = s[k];
        a_raw[(size_t)k * N + n0 + t] = s[k];
      }
    }
  }
  __syncthreads();
  // ---- per branch: chunk max, exp, sum (thread = (branch, token); the max redundantly per thread: cnt <= 32 LDS reads)
  float* out = part + (size_t)blockIdx.x * bpart_stride(K, dim);
  if (tid < K * POOL_CHUNK) {
    const int k = tid / POOL_CHUNK, t = tid % POOL_CHUNK;
    float m = -3.0e38f;
    for (int u = 0; u < cnt; ++u) m = fmaxf(m, s_a[k][u]);
    s_e[k][t] = t < cnt ? __expf(s_a[k][t] - m) : 0.f;
    if (t == 0) s_m[k] = m;
  }
  __syncthreads();
  if (tid < K) {
    float l = 0.f;
    for (int u = 0; u < cnt; ++u) l += s_e[tid][u];
    out[(size_t)K * dim + tid] = s_m[tid];
    out[(size_t)K * dim + K + tid] = l;
  }

  // ---- weighted sums of the chunk's rows (a row past the chunk meets s_e[k][31], which is 0 whenever cnt < 32)
  chunk_weighted_rowsum<K>(y, s_e, red, out, n0, cnt, dim);
}

// One block per branch: the merge core over the chunk partials, then the normalised attention row and
// the bag logits -- per_branch (CLAM_MB): logits[c] = cls_w[c] . M[c] + cls_b[c] by block c; otherwise (CLAM_SB, one branch)
// logits[j] = cls_w[j] . M[0] + cls_b[j] for the n_classes rows of the classifier.
__global__ __launch_bounds__(1024) void branch_merge_kernel(const float* __restrict__ part, const float* __restrict__ a_raw,
                                                            const float* __restrict__ cls_w, const float* __restrict__ cls_b,
                                                            float* __restrict__ pooled, float* __restrict__ logits,
                                                            float* __restrict__ attn, int per_branch, int n_classes, int N,
                                                            int dim, int K, int nb) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int br = blockIdx.x;
  // m of chunk b: (part + K * dim + br)[b * ps], l: K floats further; its row for this branch: (part + br * dim) + b * ps
  const PoolMerged p = pool_merge_core(part + (size_t)K * dim + br, K, part + (size_t)br * dim, bpart_stride(K, dim), nb, dim,
                                       smem, pooled ? pooled + (size_t)br * dim : nullptr);

  // bag logits: one wave per classifier row
  if (logits) {
    const int j0 = per_branch ? br : 0, j1 = per_branch ? br + 1 : (br == 0 ? n_classes : 0);
    for (int j = j0 + wave; j < j1; j += 16) {
      const float acc = wave_row_dot(cls_w + (size_t)j * dim, p.s_pool, dim, lane);
      if (lane == 0) logits[j] = acc + (cls_b ? cls_b[j] : 0.f);
    }
  }
  if (attn) {
    for (int n = tid; n < N; n += 1024) attn[(size_t)br * N + n] = __expf(a_raw[(size_t)br * N + n] - p.M) * p.invL;
  }
}

// ---- backward.  Given d M [K, dim] (and optionally d s [K, N] for callers that use the raw scores):
//     dA[c, n] = y_n . dM[c]        ds[c, n] = A[c, n] (dA[c, n] - M[c] . dM[c]) (+ d_raw[c, n])
//     dy_n = sum_c A[c, n] dM[c]    g_n = sum_c ds[c, n] c_w[c] ,  d hid_a = g * hid_b ,  d hid_b = g * hid_a  (d hid_a = g ungated)
//     d c_w[c] = sum_n ds[c, n] h_n     d c_b[c] = sum_n ds[c, n]
// One wave per token, BR_BWD_ROWS tokens per block; per-block partials of (d c_w [K, hid] | d c_b [K]) -> launch_reduce_partials.
constexpr int BR_BWD_ROWS = 32;
__host__ __device__ __forceinline__ size_t bbwd_stride(int K, int hid) { return (size_t)K * hid + 8; }

template <int K>
__global__ __launch_bounds__(256) void branch_backward_kernel(const float* __restrict__ y, const float* __restrict__ hid_a,
                                                              const float* __restrict__ hid_b, const float* __restrict__ wc,
                                                              const float* __restrict__ attn, const float* __restrict__ pooled,
                                                              const float* __restrict__ d_pooled, const float* __restrict__ d_raw,
                                                              float* __restrict__ dy, float* __restrict__ dhid_a,
                                                              float* __restrict__ dhid_b, float* __restrict__ part, int N, int dim,
                                                              int hid) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* s_dp = (float*)smem;                        // d M [K][dim]
  float* s_acc = s_dp + (size_t)K * dim;             // [4 waves][K * hid + 8]: this block's d c_w | d c_b partial
  __shared__ float s_c[K][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int accw = (int)bbwd_stride(K, hid);
  for (int c = tid; c < 4 * accw; c += 256) s_acc[c] = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k)
    pool_backward_stage(d_pooled + (size_t)k * dim, pooled + (size_t)k * dim, s_dp + k * dim, s_c[k], dim);
  __syncthreads();
  float cc[K], dbc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    cc[k] = pool_backward_c(s_c[k]);
    dbc[k] = 0.f;
  }
  float* myacc = s_acc + wave * accw;
  const int n0 = blockIdx.x * BR_BWD_ROWS;
  for (int t = wave; t < BR_BWD_ROWS; t += 4) {
    const int n = n0 + t;
    if (n >= N) break;
    float a[K], da[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      a[k] = attn[(size_t)k * N + n];
      da[k] = 0.f;
    }
    const float* yr = y + (size_t)n * dim;
    for (int c = lane * 4; c < dim; c += 256) {
      const float4 v = *(const float4*)(yr + c);
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const float4 d = *(const float4*)(s_dp + k * dim + c);
        da[k] += (v.x * d.x + v.y * d.y) + (v.z * d.z + v.w * d.w);
        o.x += a[k] * d.x; o.y += a[k] * d.y; o.z += a[k] * d.z; o.w += a[k] * d.w;
      }
      *(float4*)(dy + (size_t)n * dim + c) = o;
    }
    float ds[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      ds[k] = a[k] * (wave_sum(da[k]) - cc[k]) + (d_raw ? d_raw[(size_t)k * N + n] : 0.f);
      dbc[k] += ds[k];
    }
    for (int c = lane * 4; c < hid; c += 256) {
      const float4 ha = *(const float4*)(hid_a + (size_t)n * hid + c);
      float4 h = ha, hb = make_float4(1.f, 1.f, 1.f, 1.f);
      if (hid_b) {
        hb = *(const float4*)(hid_b + (size_t)n * hid + c);
        h = make_float4(ha.x * hb.x, ha.y * hb.y, ha.z * hb.z, ha.w * hb.w);
      }
      float4 g = make_float4(0.f, 0.f, 0.f, 0.f);                               // d (h_a h_b) (or d h_a)
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const float4 w = *(const float4*)(wc + (size_t)k * hid + c);
        g.x += ds[k] * w.x; g.y += ds[k] * w.y; g.z += ds[k] * w.z; g.w += ds[k] * w.w;
        float4 acc = *(float4*)(myacc + k * hid + c);
        acc.x += ds[k] * h.x; acc.y += ds[k] * h.y; acc.z += ds[k] * h.z; acc.w += ds[k] * h.w;
        *(float4*)(myacc + k * hid + c) = acc;
      }
      if (hid_b) {
        *(float4*)(dhid_b + (size_t)n * hid + c) = make_float4(g.x * ha.x, g.y * ha.y, g.z * ha.z, g.w * ha.w);
        g = make_float4(g.x * hb.x, g.y * hb.y, g.z * hb.z, g.w * hb.w);
      }
      *(float4*)(dhid_a + (size_t)n * hid + c) = g;
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) myacc[K * hid + k] = dbc[k];
  }
  __syncthreads();
  float* out = part + (size_t)blockIdx.x * accw;
  for (int c = tid; c < accw; c += 256) out[c] = (s_acc[c] + s_acc[accw + c]) + (s_acc[2 * accw + c] + s_acc[3 * accw + c]);
}

// ---- top-k of rows.  For each of K rows of N floats: the ids of the k largest (descending) and of the k smallest
// (ascending) values.  ORDER: a strict total order -- value first, LOWER INDEX first among equal values (both ends) -- so the
// result does not depend on how the row is split over waves.  NaN entries are never selected (a row with fewer than k
// other values gets -1 in its unused slots).  One pass over the row and no
// sort of it: every wave keeps the 64 best entries it has met as a sorted list with one entry per lane; a row element is
// looked at again only if it beats the wave's current k-th entry (after a short warm-up that happens ~k ln(N / k) times per
// wave), and is then inserted by a one-lane shift of the worse entries.  The four lists are merged by rank counting.
constexpr int TOPK_MAX = 32;
constexpr int TOPK_NONE = 0x7fffffff;

__device__ __forceinline__ bool tk_better(float v, int i, float w, int j) { return v > w || (v == w && i < j); }

__global__ __launch_bounds__(256) void topk_rows_kernel(const float* __restrict__ x, long long* __restrict__ out, int N, int k) {
  __shared__ float s_v[4 * TOPK_MAX];
  __shared__ int s_i[4 * TOPK_MAX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row = blockIdx.x, side = blockIdx.y;                   // side 0: largest, 1: smallest (largest of -x)
  const float* xr = x + (size_t)row * N;
  const float NEG_INF = -__builtin_huge_valf();
  float lv = NEG_INF;                                               // this lane's list entry: (value, index), best in lane 0
  int li = TOPK_NONE;
  float thr_v = NEG_INF;                                            // the list's k-th entry
  int thr_i = TOPK_NONE;
  for (int base = wave * 64; base < N; base += 256) {
    const int n = base + lane;
    float v = NEG_INF;
    int idx = TOPK_NONE;
    if (n < N) {
      const float r = xr[n];
      if (r == r) {                                                 // (NaN: never a candidate)
        v = side ? -r : r;
        idx = n;
      }
    }
    unsigned long long mask = __ballot(tk_better(v, idx, thr_v, thr_i));
    while (mask) {
      const int src = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const float nv = __shfl(v, src);
      const int ni = __shfl(idx, src);
      if (!tk_better(nv, ni, thr_v, thr_i)) continue;               // the threshold moved since the ballot (wave-uniform)
      const int pos = __popcll(__ballot(tk_better(lv, li, nv, ni)));
      const float uv = __shfl_up(lv, 1);
      const int ui = __shfl_up(li, 1);
      if (lane == pos) {
        lv = nv;
        li = ni;
      } else if (lane > pos) {
        lv = uv;
        li = ui;
      }
      thr_v = __shfl(lv, k - 1);
      thr_i = __shfl(li, k - 1);
    }
  }
  if (lane < TOPK_MAX) {
    s_v[wave * TOPK_MAX + lane] = lv;
    s_i[wave * TOPK_MAX + lane] = li;
  }
  __syncthreads();
  if (tid < 4 * TOPK_MAX) {
    const float v = s_v[tid];
    const int i = s_i[tid];
    if (i != TOPK_NONE) {
      int rank = 0;
      for (int j = 0; j < 4 * TOPK_MAX; ++j) rank += tk_better(s_v[j], s_i[j], v, i) ? 1 : 0;
      if (rank < k) out[((size_t)row * 2 + side) * k + rank] = (long long)i;
    }
  }
  if (tid < k) {                                                      // a row with fewer than k non-NaN values: -1 in the rest
    int valid = 0;
    for (int j = 0; j < 4 * TOPK_MAX; ++j) valid += s_i[j] != TOPK_NONE ? 1 : 0;
    if (tid >= valid) out[((size_t)row * 2 + side) * k + tid] = -1;
  }
}

template <int K>
hipError_t partial_k(const float* y, const float* hid_a, const float* hid_b, const float* wc, const float* bc, float* a_raw,
                     float* part, int N, int dim, int hid, int nb, hipStream_t st) {
  branch_partial_kernel<K><<<dim3(nb), dim3(256), 0, st>>>(y, hid_a, hid_b, wc, bc, a_raw, part, N, dim, hid);
  return hipGetLastError();
}

template <int K>
hipError_t backward_k(const float* y, const float* hid_a, const float* hid_b, const float* wc, const float* attn,
                      const float* pooled, const float* d_pooled, const float* d_raw, float* dy, float* dhid_a, float* dhid_b,
                      float* part, int N, int dim, int hid, int nb, size_t lds, hipStream_t st) {
  auto kern = branch_backward_kernel<K>;
  pool_raise_lds_limit((const void*)kern, lds);
  kern<<<dim3(nb), dim3(256), lds, st>>>(y, hid_a, hid_b, wc, attn, pooled, d_pooled, d_raw, dy, dhid_a, dhid_b, part, N, dim, hid);
  return hipGetLastError();
}

}  // namespace

size_t branch_pool_part_floats(int N, int dim, int K) { return (size_t)((N + POOL_CHUNK - 1) / POOL_CHUNK) * bpart_stride(K, dim); }
size_t branch_pool_backward_part_floats(int N, int hid, int K) {
  return (size_t)((N + BR_BWD_ROWS - 1) / BR_BWD_ROWS) * bbwd_stride(K, hid);
}
size_t branch_pool_backward_lds(int dim, int hid, int K) { return ((size_t)K * dim + 4 * bbwd_stride(K, hid)) * sizeof(float); }

hipError_t launch_branch_pool(const float* y, const float* hid_a, const float* hid_b, const float* wc, const float* bc,
                              const float* cls_w, const float* cls_b, float* pooled, float* logits, float* attn, float* a_raw,
                              float* part, int per_branch, int n_classes, int N, int dim, int hid, int K, hipStream_t st) {
  const int nb = (N + POOL_CHUNK - 1) / POOL_CHUNK;
  hipError_t e;
  switch (K) {
#define RRT_BR_CASE(k) \
  case k: e = partial_k<k>(y, hid_a, hid_b, wc, bc, a_raw, part, N, dim, hid, nb, st); break;
    RRT_BR_CASE(1) RRT_BR_CASE(2) RRT_BR_CASE(3) RRT_BR_CASE(4) RRT_BR_CASE(5) RRT_BR_CASE(6) RRT_BR_CASE(7) RRT_BR_CASE(8)
#undef RRT_BR_CASE
    default: return hipErrorInvalidValue;
  }
  if (e != hipSuccess) return e;
  const size_t lds = pool_merge_lds_bytes(nb, dim);
  if (lds > POOL_MERGE_LDS_MAX) return hipErrorInvalidValue;
  auto kern = branch_merge_kernel;
  pool_raise_lds_limit((const void*)kern, lds);
  kern<<<dim3(K), dim3(1024), lds, st>>>(part, a_raw, cls_w, cls_b, pooled, logits, attn, per_branch, n_classes, N, dim, K, nb);
  return hipGetLastError();
}

// d c_w [K, hid] | d c_b [K] come out as dwcb [K * hid + 8] (d c_b at [K * hid])
hipError_t launch_branch_pool_backward(const float* y, const float* hid_a, const float* hid_b, const float* wc, const float* attn,
                                       const float* pooled, const float* d_pooled, const float* d_raw, float* dy, float* dhid_a,
                                       float* dhid_b, float* dwcb, float* part, int N, int dim, int hid, int K, hipStream_t st) {
  const int nb = (N + BR_BWD_ROWS - 1) / BR_BWD_ROWS;
  const size_t lds = branch_pool_backward_lds(dim, hid, K);
  if (lds > POOL_MERGE_LDS_MAX) return hipErrorInvalidValue;
  hipError_t e;
  switch (K) {
#define RRT_BR_CASE(k) \
  case k: e = backward_k<k>(y, hid_a, hid_b, wc, attn, pooled, d_pooled, d_raw, dy, dhid_a, dhid_b, part, N, dim, hid, nb, lds, st); break;
    RRT_BR_CASE(1) RRT_BR_CASE(2) RRT_BR_CASE(3) RRT_BR_CASE(4) RRT_BR_CASE(5) RRT_BR_CASE(6) RRT_BR_CASE(7) RRT_BR_CASE(8)
#undef RRT_BR_CASE
    default: return hipErrorInvalidValue;
  }
  if (e != hipSuccess) return e;
  return launch_reduce_partials(part, dwcb, nb, bbwd_stride(K, hid), st);
}

hipError_t launch_topk_rows(const float* x, long long* out, int rows, int N, int k, hipStream_t st) {
  topk_rows_kernel<<<dim3(rows, 2), dim3(256), 0, st>>>(x, out, N, k);
  return hipGetLastError();
}
