// bag_pool.hip -- the tails of the reference's plain MIL heads around the encoder: MeanMIL (modules/mean_max.py:25-52), its
// adjoint, and IBMIL's deconfounder (modules/attmil_ibmil.py:90-101).  MaxMIL's tail is rrt_instance_max_f32 (dsmil_pool.hip),
// the attention heads' is the ABMIL pool of mil_pool.hip.
//
// Mean pool (rrt_bag_mean_f32).  The reference computes Linear(y).mean(1); the mean commutes with the Linear:
//     colmean[d] = (1/N) sum_n y[n, d] ,   logits[j] = w[j] . colmean + b[j]
// so [N, C] never exists and y [N, dim] is read ONCE with float4 loads.  colsum_chunk_kernel: a block sums MEAN_CHUNK rows
// (two row groups x 128 float4 column lanes, four rows in flight per thread) into one partial row; with more than MEAN_FAN
// partials the same kernel sums MEAN_FAN of them at a time into a second level; mean_final_kernel (one block) adds what is
// left in a fixed order, scales by 1/N and takes the C dot products.  No atomics: the same inputs give the same bits.  A NaN
// anywhere in a column reaches that column's mean and every logit.
//
// Adjoint (rrt_bag_mean_backward_f32): dy[n, :] = (1/N) sum_j d_logits[j] w[j] -- ONE row, formed in registers by the thread
// that owns its columns and stored N times, a wave writing 1 KiB of a row at a time; dW[j] = d_logits[j] colmean, db = d_logits.
//
// Deconfounder (rrt_deconf_head_f32), one block, O(J (dim + V) + K V) work, FOLDED like the DSMIL bag stream:
//     q = W_q pooled + b_q [J] ;  k_i . q = conf_i . (W_k^T q) + b_k . q   so k [K, J] is never formed;
//     a = softmax_i(k_i . q / sqrt(J)) over the K confounders ;  cf = sum_i a_i conf_i ;  logits = head [pooled | cf] + b.
#include "pool_core.h"

namespace {

// ---------------------------------------------------------------- mean pool
// out[b, :] = sum of rows [b * fan, min((b + 1) * fan, n_in)) of in [n_in, dim]; thread = (row group rg of 2, float4 column
// lane of 128); row t of the chunk belongs to group t & 1, the groups are added as (group 0) + (group 1).
__global__ __launch_bounds__(256) void colsum_chunk_kernel(const float* __restrict__ in, float* __restrict__ out, int n_in,
                                                           int fan, int dim) {
  __shared__ float4 red[128];
  const int tid = threadIdx.x, cl = tid & 127, rg = tid >> 7;
  const int n0 = blockIdx.x * fan;
  const int cnt = min(fan, n_in - n0);
  float* o = out + (size_t)blockIdx.x * dim;
  for (int cb = 0; cb < dim; cb += 512) {
    const int c = cb + cl * 4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < dim) {
      for (int t0 = rg; t0 < cnt; t0 += 8) {            // 4 independent rows in flight
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int t = t0 + 2 * u;
          v[u] = t < cnt ? *(const float4*)(in + (size_t)(n0 + t) * dim + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w;
        }
      }
    }
    if (rg == 1 && c < dim) red[cl] = acc;
    __syncthreads();
    if (rg == 0 && c < dim) {
      const float4 r = red[cl];
      *(float4*)(o + c) = make_float4(acc.x + r.x, acc.y + r.y, acc.z + r.z, acc.w + r.w);
    }
    __syncthreads();
  }
}

// One block: colmean = inv_n * (sum of the n_in partial rows) -- thread = (row group of 8, float4 column lane of 128), the
// groups added in the order 0 .. 7 -- then logits[j] = w[j] . colmean + b[j], one wave per class in turn.
__global__ __launch_bounds__(1024) void mean_final_kernel(const float* __restrict__ part, const float* __restrict__ w,
                                                          const float* __restrict__ b, float* __restrict__ colmean,
                                                          float* __restrict__ logits, int n_in, int dim, int C, float inv_n) {
  __shared__ float4 s_red[8 * 128];
  __shared__ __attribute__((aligned(16))) float s_mean[2048];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cl = tid & 127, grp = tid >> 7;
  for (int cb = 0; cb < dim; cb += 512) {
    const int c = cb + cl * 4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < dim) {
      for (int r0 = grp; r0 < n_in; r0 += 32) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int r = r0 + 8 * u;
          v[u] = r < n_in ? *(const float4*)(part + (size_t)r * dim + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w;
        }
      }
    }
    s_red[grp * 128 + cl] = acc;
    __syncthreads();
    if (grp == 0 && c < dim) {
      float4 a = s_red[cl];
#pragma unroll
      for (int q = 1; q < 8; ++q) {
        const float4 o = s_red[q * 128 + cl];
        a.x += o.x; a.y += o.y; a.z += o.z; a.w += o.w;
      }
      a.x *= inv_n; a.y *= inv_n; a.z *= inv_n; a.w *= inv_n;
      *(float4*)(s_mean + c) = a;
      if (colmean) *(float4*)(colmean + c) = a;
    }
    __syncthreads();
  }
  for (int j = wave; j < C; j += 16) {
    const float acc = wave_row_dot(w + (size_t)j * dim, s_mean, dim, lane);
    if (lane == 0) logits[j] = acc + (b ? b[j] : 0.f);
  }
}

// dy rows [blockIdx.x * MEAN_BWD_ROWS, ...): L = min(dim / 4, 256) float4 column lanes x 256 / L row groups.  Every thread
// that owns a column forms the row's value by the same expression: the rows are bit-identical.
__global__ __launch_bounds__(256) void mean_backward_kernel(const float* __restrict__ d_logits, const float* __restrict__ w,
                                                            float* __restrict__ dy, int N, int dim, int C, float inv_n) {
  const int tid = threadIdx.x;
  const int dim4 = dim >> 2;
  const int L = min(dim4, 256), RG = 256 / L;
  const int rg = tid / L, cl = tid - rg * L;
  if (rg >= RG) return;
  const int n0 = blockIdx.x * MEAN_BWD_ROWS;
  const int cnt = min(MEAN_BWD_ROWS, N - n0);
  for (int c4 = cl; c4 < dim4; c4 += L) {
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = 0; j < C; ++j) {
      const float g = d_logits[j];
      const float4 x = *(const float4*)(w + (size_t)j * dim + c4 * 4);
      r.x += g * x.x; r.y += g * x.y; r.z += g * x.z; r.w += g * x.w;
    }
    r.x *= inv_n; r.y *= inv_n; r.z *= inv_n; r.w *= inv_n;
    for (int t = rg; t < cnt; t += RG) *(float4*)(dy + (size_t)(n0 + t) * dim + c4 * 4) = r;
  }
}

// dW[j, :] = d_logits[j] * colmean, db = d_logits (one block)
__global__ __launch_bounds__(256) void mean_backward_params_kernel(const float* __restrict__ d_logits,
                                                                   const float* __restrict__ colmean, float* __restrict__ dW,
                                                                   float* __restrict__ db, int dim, int C) {
  const int tid = threadIdx.x;
  if (dW) {
    for (int i = tid; i < C * dim; i += 256) {
      const int j = i / dim;
      dW[i] = d_logits[j] * colmean[i - j * dim];
    }
  }
  if (db && tid < C) db[tid] = d_logits[tid];
}

// ---------------------------------------------------------------- IBMIL deconfounder (one block)
__global__ __launch_bounds__(256) void deconf_head_kernel(const float* __restrict__ pooled, const float* __restrict__ conf,
                                                          const float* __restrict__ q_w, const float* __restrict__ q_b,
                                                          const float* __restrict__ k_w, const float* __restrict__ k_b,
                                                          const float* __restrict__ head_w, const float* __restrict__ head_b,
                                                          float* __restrict__ logits, float* __restrict__ a_out,
                                                          float* __restrict__ cf_out, int dim, int K, int V, int J, int C,
                                                          float scale) {
  __shared__ __attribute__((aligned(16))) float s_p[2048];    // pooled [dim]
  __shared__ __attribute__((aligned(16))) float s_u[2048];    // W_k^T q [V]
  __shared__ __attribute__((aligned(16))) float s_cf[2048];   // cf [V]
  __shared__ float s_q[512];                                  // q [J]
  __shared__ float s_s[64];                                   // scores, then a [K]
  __shared__ float s_beta;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int c = tid; c < dim; c += 256) s_p[c] = pooled[c];
  __syncthreads();
  for (int j = wave; j < J; j += 4) {
    const float acc = wave_row_dot(q_w + (size_t)j * dim, s_p, dim, lane) + (q_b ? q_b[j] : 0.f);
    if (lane == 0) s_q[j] = acc;
  }
  __syncthreads();
  for (int v = tid; v < V; v += 256) {
    float acc = 0.f;
    for (int j = 0; j < J; ++j) acc += k_w[(size_t)j * V + v] * s_q[j];
    s_u[v] = acc;
  }
  if (wave == 0) {
    float acc = 0.f;
    if (k_b)
      for (int j = lane; j < J; j += 64) acc += k_b[j] * s_q[j];
    acc = wave_sum(acc);
    if (lane == 0) s_beta = acc;
  }
  __syncthreads();
  for (int i = wave; i < K; i += 4) {
    const float acc = wave_row_dot(conf + (size_t)i * V, s_u, V, lane);
    if (lane == 0) s_s[i] = (acc + s_beta) * scale;
  }
  __syncthreads();
  if (wave == 0) {                                             // softmax over the K <= 64 confounders
    const float s = lane < K ? s_s[lane] : -3.0e38f;
    const float m = wave_max(s);
    const float e = lane < K ? expf(s - m) : 0.f;
    const float l = wave_sum(e);
    const float a = e / l;
    if (lane < K) {
      s_s[lane] = a;
      if (a_out) a_out[lane] = a;
    }
  }
  __syncthreads();
  for (int v = tid; v < V; v += 256) {
    float acc = 0.f;
    for (int i = 0; i < K; ++i) acc += s_s[i] * conf[(size_t)i * V + v];
    s_cf[v] = acc;
    if (cf_out) cf_out[v] = acc;
  }
  __syncthreads();
  const size_t hs = (size_t)dim + V;
  for (int o = wave; o < C; o += 4) {
    float acc = lane_row_dot(head_w + o * hs, s_p, dim, lane, 0.f);          // [pooled | cf]: one sum over both segments
    acc = wave_sum(lane_row_dot(head_w + o * hs + dim, s_cf, V, lane, acc));
    if (lane == 0) logits[o] = acc + (head_b ? head_b[o] : 0.f);
  }
}

}  // namespace

size_t bag_mean_part1_rows(int N) { return (size_t)((N + MEAN_CHUNK - 1) / MEAN_CHUNK); }
size_t bag_mean_part2_rows(int N) { return (bag_mean_part1_rows(N) + MEAN_FAN - 1) / MEAN_FAN; }

// part1 [bag_mean_part1_rows(N), dim], part2 [bag_mean_part2_rows(N), dim]: workspace pieces (api.hip carves them)
hipError_t launch_bag_mean(const float* y, const float* w, const float* b, float* logits, float* colmean, float* part1,
                           float* part2, int N, int dim, int C, hipStream_t st) {
  if (dim > 2048 || dim % 4) return hipErrorInvalidValue;
  const int nb1 = (int)bag_mean_part1_rows(N), nb2 = (int)bag_mean_part2_rows(N);
  colsum_chunk_kernel<<<dim3(nb1), dim3(256), 0, st>>>(y, part1, N, MEAN_CHUNK, dim);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const float* last = part1;
  int n_last = nb1;
  if (nb1 > MEAN_FAN) {
    colsum_chunk_kernel<<<dim3(nb2), dim3(256), 0, st>>>(part1, part2, nb1, MEAN_FAN, dim);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    last = part2;
    n_last = nb2;
  }
  mean_final_kernel<<<dim3(1), dim3(1024), 0, st>>>(last, w, b, colmean, logits, n_last, dim, C, 1.0f / (float)N);
  return hipGetLastError();
}

hipError_t launch_bag_mean_backward(const float* d_logits, const float* colmean, const float* w, float* dy, float* dW, float* db,
                                    int N, int dim, int C, hipStream_t st) {
  if (dim % 4) return hipErrorInvalidValue;
  hipError_t e = hipSuccess;
  if (dy) {
    const int nb = (N + MEAN_BWD_ROWS - 1) / MEAN_BWD_ROWS;
    mean_backward_kernel<<<dim3(nb), dim3(256), 0, st>>>(d_logits, w, dy, N, dim, C, 1.0f / (float)N);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (dW || db) {
    mean_backward_params_kernel<<<dim3(1), dim3(256), 0, st>>>(d_logits, colmean, dW, db, dim, C);
    e = hipGetLastError();
  }
  return e;
}

hipError_t launch_deconf_head(const float* pooled, const float* conf, const float* q_w, const float* q_b, const float* k_w,
                              const float* k_b, const float* head_w, const float* head_b, float* logits, float* a, float* cf,
                              int dim, int K, int V, int J, int C, hipStream_t st) {
  if (dim > 2048 || V > 2048 || J > 512 || K < 1 || K > 64 || dim % 4 || V % 4) return hipErrorInvalidValue;
  deconf_head_kernel<<<dim3(1), dim3(256), 0, st>>>(pooled, conf, q_w, q_b, k_w, k_b, head_w, head_b, logits, a, cf, dim, K, V, J,
                                                    C, 1.0f / sqrtf((float)J));
  return hipGetLastError();
}
