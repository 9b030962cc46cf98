// segment_pool.hip -- DTFD-MIL's first tier (Survival/models/DTFD/network.py: train_forward / test_forward, the loop over
// index_chunk_list): the bag's N rows, taken in the order perm, are split into G pseudo-bags as np.array_split splits them
// (q = N / G, r = N % G: the first r groups hold q + 1 rows, the others q); every group g gets
//     w_i    = softmax over the group of a_i
//     f_g    = sum_i w_i mid_i                                                   (pooled [G, dim])
//     p_i    = softmax_c(w_i * (mid_i . Wcls_c))[C - 1]                          (get_cam_1d: the classifier's weight, no bias)
//     imax_g = argmax_i p_i ,  imin_g = argmin_i p_i                             (sel [G, 2], original row indices)
// in three launches over one read of mid: a partial per (group, chunk of POOL_CHUNK positions) -- the online-softmax triple
// (m, l, v[dim]) of pool_core.h and, from the same registers, the C dot products z_ic = mid_i . Wcls_c --, then one block per
// group that merges its partials and walks its positions for p and the two selections.  Ties: among equal p the lower
// position in group order wins at both ends, -0 = +0, a NaN p is never selected, a group whose every p is NaN selects its
// first member twice.  Everything is fp32 with accurate expf, and every sum has a fixed order: the same inputs give the same
// bits.  No atomics: every row belongs to exactly one group.
#include "pool_core.h"

namespace {

__device__ __forceinline__ size_t seg_part_stride(int dim) { return (size_t)dim + 4; }

// np.array_split in closed form: groups 0..r-1 hold q + 1 rows (c1 chunks each), the others q rows (c0 chunks each)
struct SegSplit {
  int q, r, c0, c1;
};
__host__ __device__ __forceinline__ SegSplit seg_split(int N, int G) {
  SegSplit s;
  s.q = N / G;
  s.r = N % G;
  s.c0 = (s.q + POOL_CHUNK - 1) / POOL_CHUNK;
  s.c1 = (s.q + 1 + POOL_CHUNK - 1) / POOL_CHUNK;
  return s;
}
__host__ __device__ __forceinline__ int seg_blocks(const SegSplit& s, int G) { return s.r * s.c1 + (G - s.r) * s.c0; }
__device__ __forceinline__ int seg_start(const SegSplit& s, int g) { return g * s.q + min(g, s.r); }
__device__ __forceinline__ int seg_size(const SegSplit& s, int g) { return s.q + (g < s.r ? 1 : 0); }
__device__ __forceinline__ int seg_first_part(const SegSplit& s, int g) {
  return g < s.r ? g * s.c1 : s.r * s.c1 + (g - s.r) * s.c0;
}
// block -> (group, chunk of the group)
__device__ __forceinline__ void seg_block(const SegSplit& s, int b, int& g, int& ch) {
  const int head = s.r * s.c1;
  if (b < head) {
    g = b / s.c1;
    ch = b - g * s.c1;
  } else {
    const int t = b - head;
    g = s.r + t / s.c0;
    ch = t - (t / s.c0) * s.c0;
  }
}
// the row behind group-order position j; -1 for a perm entry outside [0, N), which is never dereferenced
__device__ __forceinline__ int seg_row(const long long* __restrict__ perm, int j, int N) {
  if (!perm) return j;
  const long long i = perm[j];
  return (i < 0 || i >= N) ? -1 : (int)i;
}

// a_n = wc . h_n (+ bc): the gate score of pool_core.h as a stage of its own, one wave per row in the ABMIL pool's chunks
__global__ __launch_bounds__(256) void gate_scores_kernel(const float* __restrict__ hid_a, const float* __restrict__ hid_b,
                                                          const float* __restrict__ wc, const float* __restrict__ bc,
                                                          float* __restrict__ a_raw, int N, int hid) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * POOL_CHUNK;
  const int cnt = min(POOL_CHUNK, N - n0);
  const float b = bc ? bc[0] : 0.f;
  for (int t = wave; t < cnt; t += 4) {
    float s[1];
    gate_scores_row<1>(hid_a, hid_b, wc, (size_t)(n0 + t) * hid, hid, lane, s);
    if (lane == 0) a_raw[n0 + t] = s[0] + b;
  }
}

constexpr int SEG_MAX_DIM = 2048, SEG_MAX_C = 8;
constexpr int SEG_Q = SEG_MAX_DIM / 256;      // float4 columns a lane holds of one row

// One block per (group, chunk): one wave per row, POOL_CHUNK / 4 rows per wave; a lane holds the float4 columns
// lane * 4 + 256 * k of its row, multiplies them into the wave's running weighted sum and into the C class dot products.
// LDS: Wcls [C, dim] while the rows stream, then (the same floats) three waves' partial sums for the fixed-order add.
__global__ __launch_bounds__(256) void seg_partial_kernel(const float* __restrict__ mid, const float* __restrict__ a,
                                                          const long long* __restrict__ perm, const float* __restrict__ cls_w,
                                                          float* __restrict__ part, float* __restrict__ z, int N, int dim, int C,
                                                          int G) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* s_w = (float*)smem;                         // [max(C, 3) * dim]
  __shared__ float s_a[POOL_CHUNK];
  __shared__ float s_e[POOL_CHUNK];
  __shared__ int s_row[POOL_CHUNK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const SegSplit sp = seg_split(N, G);
  int g, ch;
  seg_block(sp, blockIdx.x, g, ch);
  const int j0 = seg_start(sp, g) + ch * POOL_CHUNK;
  const int cnt = min(POOL_CHUNK, seg_size(sp, g) - ch * POOL_CHUNK);

  for (int c = tid * 4; c < C * dim; c += 1024) *(float4*)(s_w + c) = *(const float4*)(cls_w + c);
  if (tid < cnt) {
    const int row = seg_row(perm, j0 + tid, N);
    s_row[tid] = row;
    s_a[tid] = row >= 0 ? a[row] : __builtin_nanf("");
  }
  __syncthreads();
  float m = -3.0e38f;
  for (int t = 0; t < cnt; ++t) m = fmaxf(m, s_a[t]);
  if (tid < cnt) s_e[tid] = expf(s_a[tid] - m);
  __syncthreads();
  float l = 0.f;
  for (int t = 0; t < cnt; ++t) l += s_e[t];

  float4 acc[SEG_Q];
#pragma unroll
  for (int k = 0; k < SEG_Q; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int t = wave; t < cnt; t += 4) {
    const int row = s_row[t];
    const float e = s_e[t];
    const float* src = mid + (size_t)(row >= 0 ? row : 0) * dim;
    float zc[SEG_MAX_C];
#pragma unroll
    for (int c = 0; c < SEG_MAX_C; ++c) zc[c] = 0.f;
#pragma unroll
    for (int k = 0; k < SEG_Q; ++k) {
      const int col = k * 256 + lane * 4;
      if (col < dim) {
        float4 v = *(const float4*)(src + col);
        if (row < 0) v = make_float4(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""));
        acc[k].x += e * v.x; acc[k].y += e * v.y; acc[k].z += e * v.z; acc[k].w += e * v.w;
#pragma unroll
        for (int c = 0; c < SEG_MAX_C; ++c) {
          if (c < C) {
            const float4 w = *(const float4*)(s_w + (size_t)c * dim + col);
            zc[c] += (v.x * w.x + v.y * w.y) + (v.z * w.z + v.w * w.w);
          }
        }
      }
    }
#pragma unroll
    for (int c = 0; c < SEG_MAX_C; ++c) {
      if (c < C) {
        const float s = wave_sum(zc[c]);
        if (lane == 0) z[(size_t)(j0 + t) * C + c] = s;
      }
    }
  }
  __syncthreads();                                   // Wcls is done with: its floats hold waves 1..3's sums now
  if (wave > 0) {
#pragma unroll
    for (int k = 0; k < SEG_Q; ++k) {
      const int col = k * 256 + lane * 4;
      if (col < dim) *(float4*)(s_w + (size_t)(wave - 1) * dim + col) = acc[k];
    }
  }
  __syncthreads();
  float* out = part + (size_t)blockIdx.x * seg_part_stride(dim);
  if (wave == 0) {
#pragma unroll
    for (int k = 0; k < SEG_Q; ++k) {
      const int col = k * 256 + lane * 4;
      if (col < dim) {
        const float4 o1 = *(const float4*)(s_w + col), o2 = *(const float4*)(s_w + dim + col),
                     o3 = *(const float4*)(s_w + 2 * (size_t)dim + col);
        *(float4*)(out + col) = make_float4((acc[k].x + o1.x) + (o2.x + o3.x), (acc[k].y + o1.y) + (o2.y + o3.y),
                                            (acc[k].z + o1.z) + (o2.z + o3.z), (acc[k].w + o1.w) + (o2.w + o3.w));
      }
    }
  }
  if (tid == 0) {
    out[dim] = m;
    out[dim + 1] = l;
  }
}

// (value, position) candidates of the block's threads -> the winner under the tie rule; pos < 0: the thread saw no candidate
__device__ __forceinline__ int seg_pick(const float* s_v, const int* s_p, bool largest) {
  float bv = 0.f;
  int bp = -1;
  for (int t = 0; t < 256; ++t) {
    const int p = s_p[t];
    if (p < 0) continue;
    const float v = s_v[t];
    if (bp < 0 || (largest ? v > bv : v < bv) || (v == bv && p < bp)) {
      bv = v;
      bp = p;
    }
  }
  return bp < 0 ? 0 : bp;
}

// One block per group: merge the group's partials (m_g, l_g, f_g), then walk the group's positions: w_j, p_j, argmax / argmin.
// ids (optional, [2G] or [G]): the selected rows in the layout tier 2 gathers by -- ids_stride 2: max and min, 1: max alone.
__global__ __launch_bounds__(256) void seg_merge_select_kernel(const float* __restrict__ part, const float* __restrict__ z,
                                                               const float* __restrict__ a, const long long* __restrict__ perm,
                                                               float* __restrict__ pooled, long long* __restrict__ sel,
                                                               float* __restrict__ attn, float* __restrict__ pout,
                                                               float* __restrict__ ml, long long* __restrict__ ids,
                                                               int ids_stride, int N, int dim, int C, int G) {
  __shared__ float s_red[4];
  __shared__ float s_M, s_invL;
  __shared__ float4 s_half[128];
  __shared__ float s_vmax[256], s_vmin[256];
  __shared__ int s_pmax[256], s_pmin[256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = blockIdx.x;
  const SegSplit sp = seg_split(N, G);
  const int start = seg_start(sp, g), size = seg_size(sp, g);
  const int nb = g < sp.r ? sp.c1 : sp.c0;
  const size_t ps = seg_part_stride(dim);
  const float* gp = part + (size_t)seg_first_part(sp, g) * ps;

  float m = -3.0e38f;
  for (int b = tid; b < nb; b += 256) m = fmaxf(m, gp[b * ps + dim]);
  m = wave_max(m);
  if (lane == 0) s_red[wave] = m;
  __syncthreads();
  if (tid == 0) s_M = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
  __syncthreads();
  const float M = s_M;
  float l = 0.f;
  for (int b = tid; b < nb; b += 256) l += gp[b * ps + dim + 1] * expf(gp[b * ps + dim] - M);
  l = wave_sum(l);
  if (lane == 0) s_red[wave] = l;
  __syncthreads();
  if (tid == 0) {
    const float L = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
    s_invL = 1.0f / L;
    ml[2 * g] = M;
    ml[2 * g + 1] = L;
  }
  __syncthreads();
  const float invL = s_invL;

  // f_g[c] = invL * sum_b exp(m_b - M) v_b[c]: thread = (half of the partials, float4 column lane of 128)
  const int cl = tid & 127, half = tid >> 7;
  for (int cb = 0; cb < dim; cb += 512) {
    const int c = cb + cl * 4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < dim) {
      for (int b = half; b < nb; b += 2) {
        const float sc = expf(gp[b * ps + dim] - M);
        const float4 v = *(const float4*)(gp + b * ps + c);
        acc.x += sc * v.x; acc.y += sc * v.y; acc.z += sc * v.z; acc.w += sc * v.w;
      }
    }
    if (half == 1) s_half[cl] = acc;
    __syncthreads();
    if (half == 0 && c < dim) {
      const float4 o = s_half[cl];
      *(float4*)(pooled + (size_t)g * dim + c) =
          make_float4((acc.x + o.x) * invL, (acc.y + o.y) * invL, (acc.z + o.z) * invL, (acc.w + o.w) * invL);
    }
    __syncthreads();
  }

  // the positions of the group: a thread meets its positions in rising order, so a strict comparison keeps the lower one
  float vmax = 0.f, vmin = 0.f;
  int pmax = -1, pmin = -1;
  for (int j = tid; j < size; j += 256) {
    const int row = seg_row(perm, start + j, N);
    const float w = row >= 0 ? expf(a[row] - M) * invL : __builtin_nanf("");
    float lg[SEG_MAX_C];
    float mx = -3.0e38f;
#pragma unroll
    for (int c = 0; c < SEG_MAX_C; ++c) {
      if (c < C) {
        lg[c] = w * z[(size_t)(start + j) * C + c];
        mx = fmaxf(mx, lg[c]);
      }
    }
    float den = 0.f, last = 0.f;
#pragma unroll
    for (int c = 0; c < SEG_MAX_C; ++c) {
      if (c < C) {
        last = expf(lg[c] - mx);       // (a NaN logit: fmaxf skipped it, expf carries it into den)
        den += last;
      }
    }
    const float p = last / den;
    if (row >= 0) {
      if (attn) attn[row] = w;
      if (pout) pout[row] = p;
    }
    if (p == p) {
      if (pmax < 0 || p > vmax) {
        vmax = p;
        pmax = j;
      }
      if (pmin < 0 || p < vmin) {
        vmin = p;
        pmin = j;
      }
    }
  }
  s_vmax[tid] = vmax;
  s_pmax[tid] = pmax;
  s_vmin[tid] = vmin;
  s_pmin[tid] = pmin;
  __syncthreads();
  if (tid == 0 || tid == 64) {
    const bool largest = tid == 0;
    const int pos = largest ? seg_pick(s_vmax, s_pmax, true) : seg_pick(s_vmin, s_pmin, false);
    const long long row = seg_row(perm, start + pos, N);
    sel[2 * g + (largest ? 0 : 1)] = row;
    if (ids && (largest || ids_stride == 2)) ids[(size_t)ids_stride * g + (largest ? 0 : 1)] = row;
  }
}

// Adjoint of the pooling: with c_g = pooled_g . d_pooled_g,  d_mid_i = w_i d_pooled_g ,  d_a_i = w_i (mid_i . d_pooled_g - c_g).
// The forward's grid: one block per (group, chunk), one wave per row; (m_g, l_g) as the forward left them.
__global__ __launch_bounds__(256) void seg_backward_kernel(const float* __restrict__ mid, const float* __restrict__ a,
                                                           const long long* __restrict__ perm, const float* __restrict__ pooled,
                                                           const float* __restrict__ d_pooled, const float* __restrict__ ml,
                                                           float* __restrict__ d_mid, float* __restrict__ d_a, int N, int dim,
                                                           int G) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* s_dp = (float*)smem;                        // [dim]
  __shared__ float s_c[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const SegSplit sp = seg_split(N, G);
  int g, ch;
  seg_block(sp, blockIdx.x, g, ch);
  const int j0 = seg_start(sp, g) + ch * POOL_CHUNK;
  const int cnt = min(POOL_CHUNK, seg_size(sp, g) - ch * POOL_CHUNK);
  pool_backward_stage(d_pooled + (size_t)g * dim, pooled + (size_t)g * dim, s_dp, s_c, dim);
  __syncthreads();
  const float cc = pool_backward_c(s_c);
  const float M = ml[2 * g], invL = 1.0f / ml[2 * g + 1];
  for (int t = wave; t < cnt; t += 4) {
    const int row = seg_row(perm, j0 + t, N);
    if (row < 0) continue;
    const float w = expf(a[row] - M) * invL;
    const float* src = mid + (size_t)row * dim;
    float* dst = d_mid + (size_t)row * dim;
    float da = 0.f;
    for (int c = lane * 4; c < dim; c += 256) {
      const float4 v = *(const float4*)(src + c);
      const float4 d = *(const float4*)(s_dp + c);
      da += (v.x * d.x + v.y * d.y) + (v.z * d.z + v.w * d.w);
      *(float4*)(dst + c) = make_float4(w * d.x, w * d.y, w * d.z, w * d.w);
    }
    da = wave_sum(da);
    if (lane == 0) d_a[row] = w * (da - cc);
  }
}

}  // namespace

hipError_t launch_gate_scores(const float* hid_a, const float* hid_b, const float* wc, const float* bc, float* a, int N, int hid,
                              hipStream_t st) {
  gate_scores_kernel<<<dim3((N + POOL_CHUNK - 1) / POOL_CHUNK), dim3(256), 0, st>>>(hid_a, hid_b, wc, bc, a, N, hid);
  return hipGetLastError();
}

size_t segment_pool_parts(int N, int G) { return (size_t)seg_blocks(seg_split(N, G), G); }

hipError_t launch_segment_pool(const float* mid, const float* a, const long long* perm, const float* cls_w, float* pooled,
                               long long* sel, float* attn, float* p, float* ml, float* part, float* z, long long* ids,
                               int ids_stride, int N, int dim, int C, int G, hipStream_t st) {
  const int nb = (int)segment_pool_parts(N, G);
  const size_t lds = (size_t)(C > 3 ? C : 3) * dim * sizeof(float);      // <= 8 * 2048 * 4 = 64 KiB, beside 384 static bytes
  if (lds + 1024 > POOL_LDS_DEFAULT)
    (void)hipFuncSetAttribute((const void*)seg_partial_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  seg_partial_kernel<<<dim3(nb), dim3(256), lds, st>>>(mid, a, perm, cls_w, part, z, N, dim, C, G);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  seg_merge_select_kernel<<<dim3(G), dim3(256), 0, st>>>(part, z, a, perm, pooled, sel, attn, p, ml, ids, ids_stride, N, dim, C,
                                                         G);
  return hipGetLastError();
}

hipError_t launch_segment_pool_backward(const float* mid, const float* a, const long long* perm, const float* pooled,
                                        const float* d_pooled, const float* ml, float* d_mid, float* d_a, int N, int dim, int G,
                                        hipStream_t st) {
  const int nb = (int)segment_pool_parts(N, G);
  seg_backward_kernel<<<dim3(nb), dim3(256), (size_t)dim * sizeof(float), st>>>(mid, a, perm, pooled, d_pooled, ml, d_mid, d_a, N,
                                                                                dim, G);
  return hipGetLastError();
}
