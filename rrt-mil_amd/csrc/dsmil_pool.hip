// dsmil_pool.hip -- the two streams of DSMIL's MILNet (modules/dsmil.py:44-57 IClassifier's Linear, :78-94 BClassifier,
// :123-126) around the encoder.
//
// Instance stream (rrt_instance_max_f32): classes[n, j] = y_n . w[j] + b[j]; per class column its maximum and the row that
// holds it (the "critical instance", dsmil.py:84-85 sorts the whole column for it).  ORDER: value first, LOWER INDEX among equal
// values (a strict total order, so the result does not depend on how the rows are split over waves and blocks); NaN is never
// a candidate; a column without any candidate gives index 0 and a NaN maximum.
//
// Bag stream (rrt_dsmil_pool_f32), FOLDED: with m_c the critical instance of class c and q(.) = q_w . + q_b,
//     s[n, c] = q(feats_n) . q(feats[m_c]) / sqrt(Q) = feats_n . v_c + beta_c ,
//     v_c = q_w^T q(feats[m_c]) / sqrt(Q)   [dim] ,   beta_c = q_b . q(feats[m_c]) / sqrt(Q)
// so Q [N, 128] is never formed: C dot products per row instead of 128.  dsmil_prep_kernel builds v, beta from the
// device-resident indices (one block per class); dsmil_partial_kernel streams feats ONCE -- a wave owns a DS_CHUNK-token
// chunk, holds each row in registers for the scores and for the pooling, and keeps an online softmax (m, l, sum e^{s-m} f)
// per class; dsmil_merge_kernel (one block per class) merges the chunk records (pool_core.h: pool_merge_core), writes
// B[c], A[:, c] and the class's share of the Conv1d(C, C, kernel_size = dim) logits; dsmil_logits_kernel adds the C shares.
// No atomics anywhere: the same inputs give the same bits.
#include "pool_core.h"

namespace {

constexpr int IMAX_NONE = 0x7fffffff;
__device__ __forceinline__ bool im_better(float v, int i, float w, int j) { return v > w || (v == w && i < j); }

// ---------------------------------------------------------------- instance stream
// block = 4 waves = IMAX_CHUNK tokens, one wave per token in turn; per block one (max, index) record per class
template <int K>
__global__ __launch_bounds__(256) void imax_partial_kernel(const float* __restrict__ y, const float* __restrict__ w,
                                                           const float* __restrict__ b, float* __restrict__ classes,
                                                           float* __restrict__ pv, int* __restrict__ pi, int N, int dim) {
  __shared__ float s_v[4][K];
  __shared__ int s_i[4][K];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * IMAX_CHUNK;
  const int cnt = min(IMAX_CHUNK, N - n0);
  const float NEG_INF = -__builtin_huge_valf();
  float bv[K];
  int bi[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    bv[k] = NEG_INF;
    bi[k] = IMAX_NONE;
  }
  for (int t = wave; t < cnt; t += 4) {
    const float* row = y + (size_t)(n0 + t) * dim;
    float acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.f;
    for (int c = lane * 4; c < dim; c += 256) {
      const float4 h = *(const float4*)(row + c);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const float4 x = *(const float4*)(w + (size_t)k * dim + c);
        acc[k] += (h.x * x.x + h.y * x.y) + (h.z * x.z + h.w * x.w);
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float s = wave_sum(acc[k]) + (b ? b[k] : 0.f);            // (the same value in every lane)
      if (classes && lane == 0) classes[(size_t)(n0 + t) * K + k] = s;
      if (s == s && im_better(s, n0 + t, bv[k], bi[k])) {
        bv[k] = s;
        bi[k] = n0 + t;
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      s_v[wave][k] = bv[k];
      s_i[wave][k] = bi[k];
    }
  }
  __syncthreads();
  if (tid < K) {
    float v = s_v[0][tid];
    int i = s_i[0][tid];
    for (int q = 1; q < 4; ++q) {
      if (s_i[q][tid] != IMAX_NONE && im_better(s_v[q][tid], s_i[q][tid], v, i)) {
        v = s_v[q][tid];
        i = s_i[q][tid];
      }
    }
    pv[(size_t)blockIdx.x * K + tid] = v;
    pi[(size_t)blockIdx.x * K + tid] = i;
  }
}

// one block: the best record of every class over the nb block records
__global__ __launch_bounds__(256) void imax_merge_kernel(const float* __restrict__ pv, const int* __restrict__ pi,
                                                         float* __restrict__ cmax, long long* __restrict__ argmax, int K, int nb) {
  __shared__ float s_v[8][256];
  __shared__ int s_i[8][256];
  const int tid = threadIdx.x;
  for (int k = 0; k < K; ++k) {
    float v = -__builtin_huge_valf();
    int i = IMAX_NONE;
    for (int b = tid; b < nb; b += 256) {
      const float x = pv[(size_t)b * K + k];
      const int xi = pi[(size_t)b * K + k];
      if (xi != IMAX_NONE && im_better(x, xi, v, i)) {
        v = x;
        i = xi;
      }
    }
    s_v[k][tid] = v;
    s_i[k][tid] = i;
  }
  __syncthreads();
  if (tid < K) {
    float v = s_v[tid][0];
    int i = s_i[tid][0];
    for (int q = 1; q < 256; ++q) {
      if (s_i[tid][q] != IMAX_NONE && im_better(s_v[tid][q], s_i[tid][q], v, i)) {
        v = s_v[tid][q];
        i = s_i[tid][q];
      }
    }
    const bool none = i == IMAX_NONE;
    if (cmax) cmax[tid] = none ? __builtin_nanf("") : v;
    argmax[tid] = none ? 0 : (long long)i;
  }
}

// ---------------------------------------------------------------- bag stream
// part layout per chunk, as the branch pool's: [K][dim] weighted sums, then m[K], l[K] (padded: K * dim + 16 floats)
__host__ __device__ __forceinline__ size_t dpart_stride(int K, int dim) { return (size_t)K * dim + 16; }

// one block per class: q_max = q(feats[m_c]) into LDS, then v_c and beta_c.  An index outside the bag is clamped into it
// (the kernel never reads outside feats, whatever the index buffer holds).
__global__ __launch_bounds__(256) void dsmil_prep_kernel(const float* __restrict__ feats, const long long* __restrict__ argmax,
                                                         const float* __restrict__ q_w, const float* __restrict__ q_b,
                                                         float* __restrict__ v, float* __restrict__ vb, int N, int dim, int Q,
                                                         float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* s_q = (float*)smem;                         // [Q]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = blockIdx.x;
  const long long mi = argmax[c];
  const int m = mi < 0 ? 0 : (mi >= (long long)N ? N - 1 : (int)mi);
  const float* row = feats + (size_t)m * dim;
  for (int q = wave; q < Q; q += 4) {
    float a = 0.f;
    for (int cc = lane * 4; cc < dim; cc += 256) {
      const float4 h = *(const float4*)(row + cc);
      const float4 x = *(const float4*)(q_w + (size_t)q * dim + cc);
      a += (h.x * x.x + h.y * x.y) + (h.z * x.z + h.w * x.w);
    }
    a = wave_sum(a) + (q_b ? q_b[q] : 0.f);
    if (lane == 0) s_q[q] = a;
  }
  __syncthreads();
  for (int j = tid; j < dim; j += 256) {
    float a = 0.f;
    for (int q = 0; q < Q; ++q) a += q_w[(size_t)q * dim + j] * s_q[q];
    v[(size_t)c * dim + j] = a * scale;
  }
  if (wave == 0) {
    float a = 0.f;
    if (q_b)
      for (int q = lane; q < Q; q += 64) a += q_b[q] * s_q[q];
    a = wave_sum(a);
    if (lane == 0) vb[c] = a * scale;
  }
}

// One wave = one DS_CHUNK-token chunk.  NC float4 column groups per lane (column (j * 64 + lane) * 4), G rows in flight.
// A row is loaded once into registers and feeds the K scores and then the K accumulators.
template <int K, int NC, int G>
__global__ __launch_bounds__(64) void dsmil_partial_kernel(const float* __restrict__ feats, const float* __restrict__ v,
                                                           const float* __restrict__ vb, float* __restrict__ raw,
                                                           float* __restrict__ part, int N, int dim) {
  const int lane = threadIdx.x;
  const int n0 = blockIdx.x * DS_CHUNK;
  const int cnt = min(DS_CHUNK, N - n0);
  float m[K], l[K], beta[K];
  float4 acc[K][NC];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    m[k] = -3.0e38f;
    l[k] = 0.f;
    beta[k] = vb[k];
#pragma unroll
    for (int j = 0; j < NC; ++j) acc[k][j] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  for (int t0 = 0; t0 < cnt; t0 += G) {
    float4 r[G][NC];
#pragma unroll
    for (int u = 0; u < G; ++u) {
      const bool ok = t0 + u < cnt;
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        const int c = (j * 64 + lane) * 4;
        r[u][j] = (ok && c < dim) ? *(const float4*)(feats + (size_t)(n0 + t0 + u) * dim + c) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    float s[G][K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float4 w[NC];
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        const int c = (j * 64 + lane) * 4;
        w[j] = c < dim ? *(const float4*)(v + (size_t)k * dim + c) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int u = 0; u < G; ++u) {
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < NC; ++j) a += (r[u][j].x * w[j].x + r[u][j].y * w[j].y) + (r[u][j].z * w[j].z + r[u][j].w * w[j].w);
        s[u][k] = wave_sum(a) + beta[k];
      }
    }
    if (lane < G * K) {                               // lane (u, k) stores score (u, k)
      const int u = lane / K, k = lane % K;
      float x = 0.f;
#pragma unroll
      for (int uu = 0; uu < G; ++uu)
#pragma unroll
        for (int kk = 0; kk < K; ++kk) x = (uu == u && kk == k) ? s[uu][kk] : x;
      if (t0 + u < cnt) raw[(size_t)(n0 + t0 + u) * K + k] = x;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float mn = m[k];
#pragma unroll
      for (int u = 0; u < G; ++u) mn = (t0 + u < cnt) ? fmaxf(mn, s[u][k]) : mn;
      const float sc = __expf(m[k] - mn);
      m[k] = mn;
      l[k] *= sc;
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        acc[k][j].x *= sc; acc[k][j].y *= sc; acc[k][j].z *= sc; acc[k][j].w *= sc;
      }
#pragma unroll
      for (int u = 0; u < G; ++u) {
        const float e = (t0 + u < cnt) ? __expf(s[u][k] - mn) : 0.f;
        l[k] += e;
#pragma unroll
        for (int j = 0; j < NC; ++j) {
          acc[k][j].x += e * r[u][j].x; acc[k][j].y += e * r[u][j].y; acc[k][j].z += e * r[u][j].z; acc[k][j].w += e * r[u][j].w;
        }
      }
    }
  }
  float* out = part + (size_t)blockIdx.x * dpart_stride(K, dim);
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const int c = (j * 64 + lane) * 4;
      if (c < dim) *(float4*)(out + (size_t)k * dim + c) = acc[k][j];
    }
    if (lane == 0) {
      out[(size_t)K * dim + k] = m[k];
      out[(size_t)K * dim + K + k] = l[k];
    }
  }
}

// One block per class c: the merge core over the chunk records leaves B[c] in LDS; then A[:, c] in the reference's
// [N, C] layout, and this class's share of the logits: lpart[c][o] = fcc_w[o, c, :] . B[c].
__global__ __launch_bounds__(1024) void dsmil_merge_kernel(const float* __restrict__ part, const float* __restrict__ raw,
                                                           const float* __restrict__ fcc_w, float* __restrict__ B,
                                                           float* __restrict__ A, float* __restrict__ lpart, int N, int dim,
                                                           int K, int nb) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int br = blockIdx.x;
  // m of chunk b: (part + K * dim + br)[b * ps], l: K floats further; its row for this class: (part + br * dim) + b * ps
  const PoolMerged p = pool_merge_core(part + (size_t)K * dim + br, K, part + (size_t)br * dim, dpart_stride(K, dim), nb, dim,
                                       smem, B ? B + (size_t)br * dim : nullptr);

  // fcc (Conv1d(C, C, kernel_size = dim) on [1, C, dim]): output o takes fcc_w[o, c, :] . B[c] from this class -- one wave per o
  for (int o = wave; o < K; o += 16) {
    const float acc = wave_row_dot(fcc_w + ((size_t)o * K + br) * dim, p.s_pool, dim, lane);
    if (lane == 0) lpart[br * 8 + o] = acc;
  }
  if (A) {
    for (int n = tid; n < N; n += 1024) A[(size_t)n * K + br] = __expf(raw[(size_t)n * K + br] - p.M) * p.invL;
  }
}

__global__ __launch_bounds__(64) void dsmil_logits_kernel(const float* __restrict__ lpart, const float* __restrict__ fcc_b,
                                                          float* __restrict__ logits, int K) {
  const int o = threadIdx.x;
  if (o < K) {
    float a = fcc_b ? fcc_b[o] : 0.f;
    for (int c = 0; c < K; ++c) a += lpart[c * 8 + o];
    logits[o] = a;
  }
}

template <int K>
hipError_t imax_k(const float* y, const float* w, const float* b, float* classes, float* pv, int* pi, int N, int dim, int nb,
                  hipStream_t st) {
  imax_partial_kernel<K><<<dim3(nb), dim3(256), 0, st>>>(y, w, b, classes, pv, pi, N, dim);
  return hipGetLastError();
}

template <int K>
hipError_t dpartial_k(const float* feats, const float* v, const float* vb, float* raw, float* part, int N, int dim, int nb,
                      hipStream_t st) {
  if (dim <= 512)
    dsmil_partial_kernel<K, 2, 4><<<dim3(nb), dim3(64), 0, st>>>(feats, v, vb, raw, part, N, dim);
  else
    dsmil_partial_kernel<K, 8, 1><<<dim3(nb), dim3(64), 0, st>>>(feats, v, vb, raw, part, N, dim);
  return hipGetLastError();
}

}  // namespace

size_t instance_max_part_records(int N) { return (size_t)((N + IMAX_CHUNK - 1) / IMAX_CHUNK); }
size_t dsmil_pool_part_floats(int N, int dim, int K) { return (size_t)((N + DS_CHUNK - 1) / DS_CHUNK) * dpart_stride(K, dim); }

hipError_t launch_instance_max(const float* y, const float* w, const float* b, float* classes, float* cmax, long long* argmax,
                               float* pv, int* pi, int N, int dim, int K, hipStream_t st) {
  const int nb = (N + IMAX_CHUNK - 1) / IMAX_CHUNK;
  hipError_t e;
  switch (K) {
#define RRT_IM_CASE(k) \
  case k: e = imax_k<k>(y, w, b, classes, pv, pi, N, dim, nb, st); break;
    RRT_IM_CASE(1) RRT_IM_CASE(2) RRT_IM_CASE(3) RRT_IM_CASE(4) RRT_IM_CASE(5) RRT_IM_CASE(6) RRT_IM_CASE(7) RRT_IM_CASE(8)
#undef RRT_IM_CASE
    default: return hipErrorInvalidValue;
  }
  if (e != hipSuccess) return e;
  imax_merge_kernel<<<dim3(1), dim3(256), 0, st>>>(pv, pi, cmax, argmax, K, nb);
  return hipGetLastError();
}

// v [K, dim], vb [16], raw [N, K], lpart [64], part: workspace pieces (api.hip carves them)
hipError_t launch_dsmil_pool(const float* feats, const long long* argmax, const float* q_w, const float* q_b, const float* fcc_w,
                             const float* fcc_b, float* logits, float* A, float* B, float* raw, float* v, float* vb, float* lpart,
                             float* part, int N, int dim, int Q, int K, hipStream_t st) {
  const int nb = (N + DS_CHUNK - 1) / DS_CHUNK;
  const size_t lds = pool_merge_lds_bytes(nb, dim);
  if (K < 1 || K > 8 || lds > POOL_MERGE_LDS_MAX || (size_t)Q * sizeof(float) > 48 * 1024) return hipErrorInvalidValue;
  dsmil_prep_kernel<<<dim3(K), dim3(256), (size_t)Q * sizeof(float), st>>>(feats, argmax, q_w, q_b, v, vb, N, dim, Q,
                                                                         1.0f / sqrtf((float)Q));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  switch (K) {
#define RRT_DS_CASE(k) \
  case k: e = dpartial_k<k>(feats, v, vb, raw, part, N, dim, nb, st); break;
    RRT_DS_CASE(1) RRT_DS_CASE(2) RRT_DS_CASE(3) RRT_DS_CASE(4) RRT_DS_CASE(5) RRT_DS_CASE(6) RRT_DS_CASE(7) RRT_DS_CASE(8)
#undef RRT_DS_CASE
    default: return hipErrorInvalidValue;
  }
  if (e != hipSuccess) return e;
  auto kern = dsmil_merge_kernel;
  pool_raise_lds_limit((const void*)kern, lds);
  kern<<<dim3(K), dim3(1024), lds, st>>>(part, raw, fcc_w, B, A, lpart, N, dim, K, nb);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  dsmil_logits_kernel<<<dim3(1), dim3(64), 0, st>>>(lpart, fcc_b, logits, K);
  return hipGetLastError();
}
