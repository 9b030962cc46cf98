// pool_core.h -- the device pieces the attention-pooling heads share (mil_pool.hip: ABMIL, clam_pool.hip: CLAM,
// dsmil_pool.hip: DSMIL, segment_pool.hip: DTFD, bag_pool.hip: the plain heads).  The softmax over the N tokens of a bag is an
// online softmax over 32-token chunks: a chunk emits (m, l, sum e^{s-m} y) and one 1024-thread block merges the chunks.  Every
// head owns its kernels, its workspace layout and what it does with the pooled row; the arithmetic below is one copy, so
// tests/test_mil_pool_matrix.py, which holds the ABMIL kernels to float64 at every loop edge, holds it for all of them.
// Every sum has a fixed order (no atomics): the same inputs give the same bits.
#pragma once
#include "internal.h"

// One wave: sum_c w[c] x[c] over dim floats (dim % 4 == 0, both 16-byte aligned; x usually an LDS vector, w a weight row).
// lane_row_dot adds the lane's share to acc, so that two segments can meet in one wave_sum; wave_row_dot is the total.
__device__ __forceinline__ float lane_row_dot(const float* __restrict__ w, const float* __restrict__ x, int dim, int lane,
                                              float acc) {
  for (int c = lane * 4; c < dim; c += 256) {
    const float4 a = *(const float4*)(w + c);
    const float4 p = *(const float4*)(x + c);
    acc += (a.x * p.x + a.y * p.y) + (a.z * p.z + a.w * p.w);
  }
  return acc;
}
__device__ __forceinline__ float wave_row_dot(const float* __restrict__ w, const float* __restrict__ x, int dim, int lane) {
  return wave_sum(lane_row_dot(w, x, dim, lane, 0.f));
}

// One wave: the K gate scores of hidden row `row` (an offset in floats) without their bias, s[k] = wc[k] . h with h = hid_a[row]
// or hid_a[row] * hid_b[row] (gated).  The hidden row is read once for the K score rows; s is the same in every lane.  The
// caller adds bc[k]: a kernel with one score row loads it once, ahead of its loop over the tokens.
template <int K>
__device__ __forceinline__ void gate_scores_row(const float* __restrict__ hid_a, const float* __restrict__ hid_b,
                                                const float* __restrict__ wc, size_t row, int hid, int lane,
                                                float (&s)[K]) {
  float acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.f;
  for (int c = lane * 4; c < hid; c += 256) {
    float4 h = *(const float4*)(hid_a + row + c);
    if (hid_b) {
      const float4 g = *(const float4*)(hid_b + row + c);
      h.x *= g.x; h.y *= g.y; h.z *= g.z; h.w *= g.w;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float4 w = *(const float4*)(wc + (size_t)k * hid + c);
      acc[k] += (h.x * w.x + h.y * w.y) + (h.z * w.z + h.w * w.w);
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = wave_sum(acc[k]);
}

// A 256-thread block: out[k][c] = sum_{t < cnt} s_e[k][t] y[n0 + t][c] for the chunk's cnt <= POOL_CHUNK rows and K weight
// rows, out[k] at out + k * dim.  thread = (row group rg of 2, float4 column lane of 128); every row's float4 is loaded once
// and feeds the K accumulators; row t belongs to group t & 1, the groups are added as (group 0) + (group 1) through red.
// s_e[k][t] must be 0 for cnt <= t < POOL_CHUNK: a row past the chunk is zero data against the finite weight s_e[k][31].
template <int K>
__device__ __forceinline__ void chunk_weighted_rowsum(const float* __restrict__ y, const float (*s_e)[POOL_CHUNK],
                                                      float4 (*red)[128], float* __restrict__ out, int n0, int cnt, int dim) {
  const int tid = threadIdx.x, cl = tid & 127, rg = tid >> 7;
  for (int cb = 0; cb < dim; cb += 512) {
    const int c = cb + cl * 4;
    float4 acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < dim) {
      for (int t0 = rg; t0 < cnt; t0 += 8) {          // 4 independent rows in flight
        float4 v[4];
        int tt[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int t = t0 + 2 * u;
          const bool ok = t < cnt;
          tt[u] = ok ? t : POOL_CHUNK - 1;
          v[u] = ok ? *(const float4*)(y + (size_t)(n0 + t) * dim + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
          for (int k = 0; k < K; ++k) {
            const float e = s_e[k][tt[u]];
            acc[k].x += e * v[u].x; acc[k].y += e * v[u].y; acc[k].z += e * v[u].z; acc[k].w += e * v[u].w;
          }
        }
      }
    }
    if (rg == 1 && c < dim) {
#pragma unroll
      for (int k = 0; k < K; ++k) red[k][cl] = acc[k];
    }
    __syncthreads();
    if (rg == 0 && c < dim) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const float4 o = red[k][cl];
        *(float4*)(out + (size_t)k * dim + c) = make_float4(acc[k].x + o.x, acc[k].y + o.y, acc[k].z + o.z, acc[k].w + o.w);
      }
    }
    __syncthreads();
  }
}

// A 1024-thread block merges nb chunk records into one softmax-weighted row.  pm[b * ps] is chunk b's maximum m_b,
// pm[b * ps + l_off] its sum l_b, pv + b * ps its weighted row sum_t e^{s_t - m_b} y_t [dim].  With M = max_b m_b and
// L = sum_b l_b e^{m_b - M}:  pooled = (1 / L) sum_b e^{m_b - M} v_b, left in s_pool (and in gout, if given) for every thread
// after the last barrier.  smem: the block's dynamic LDS, pool_merge_lds_bytes(nb, dim) bytes.
struct PoolMerged {
  const float* s_pool;   // [dim], LDS
  float M, invL;         // a raw score s becomes the attention weight exp(s - M) * invL
};
__device__ __forceinline__ PoolMerged pool_merge_core(const float* __restrict__ pm, int l_off, const float* __restrict__ pv,
                                                      size_t ps, int nb, int dim, char* smem, float* __restrict__ gout) {
  float* s_scale = (float*)smem;                    // [nb] exp(m_b - M)
  float* s_pool = s_scale + ((nb + 3) & ~3);        // [dim]
  float4* s_red = (float4*)(s_pool + dim);          // [8 groups][128 column lanes]
  __shared__ float s_w[16];
  __shared__ float s_M, s_invL;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  float m = -3.0e38f;
  for (int b = tid; b < nb; b += 1024) m = fmaxf(m, pm[b * ps]);
  m = wave_max(m);
  if (lane == 0) s_w[wave] = m;
  __syncthreads();
  if (tid == 0) {
    float M = s_w[0];
    for (int w = 1; w < 16; ++w) M = fmaxf(M, s_w[w]);
    s_M = M;
  }
  __syncthreads();
  const float M = s_M;
  float l = 0.f;
  for (int b = tid; b < nb; b += 1024) {
    const float sc = __expf(pm[b * ps] - M);
    s_scale[b] = sc;
    l += pm[b * ps + l_off] * sc;
  }
  l = wave_sum(l);
  __syncthreads();                                  // s_w reuse
  if (lane == 0) s_w[wave] = l;
  __syncthreads();
  if (tid == 0) {
    float L = 0.f;
    for (int w = 0; w < 16; ++w) L += s_w[w];
    s_invL = 1.0f / L;
  }
  __syncthreads();
  const float invL = s_invL;

  // pooled[c] = invL * sum_b scale_b v_b[c] : thread = (chunk group of 8, float4 column lane of 128)
  const int cl = tid & 127, grp = tid >> 7;
  for (int cb = 0; cb < dim; cb += 512) {
    const int c = cb + cl * 4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < dim) {
      for (int b0 = grp; b0 < nb; b0 += 32) {
        float4 v[4];
        float sc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int b = b0 + 8 * u;
          const bool ok = b < nb;
          sc[u] = ok ? s_scale[b] : 0.f;
          v[u] = ok ? *(const float4*)(pv + b * ps + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          acc.x += sc[u] * v[u].x; acc.y += sc[u] * v[u].y; acc.z += sc[u] * v[u].z; acc.w += sc[u] * v[u].w;
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
      a.x *= invL; a.y *= invL; a.z *= invL; a.w *= invL;
      *(float4*)(s_pool + c) = a;
      if (gout) *(float4*)(gout + c) = a;
    }
    __syncthreads();
  }
  PoolMerged r;
  r.s_pool = s_pool;
  r.M = M;
  r.invL = invL;
  return r;
}

// Prologue of the pooling adjoints, a 256-thread block: d_pooled [dim] -> s_dp (LDS) and this wave's share of
// c = pooled . d_pooled -> s_c[wave].  After the caller's barrier, pool_backward_c(s_c) is c in every thread.
__device__ __forceinline__ void pool_backward_stage(const float* __restrict__ d_pooled, const float* __restrict__ pooled,
                                                    float* s_dp, float* s_c, int dim) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float cpart = 0.f;
  for (int c = tid; c < dim; c += 256) {
    const float v = d_pooled[c];
    s_dp[c] = v;
    cpart += v * pooled[c];
  }
  cpart = wave_sum(cpart);
  if (lane == 0) s_c[wave] = cpart;
}
__device__ __forceinline__ float pool_backward_c(const float* s_c) { return (s_c[0] + s_c[1]) + (s_c[2] + s_c[3]); }
