// transmil_bwd.hip -- what TransMIL's one-call training step needs besides the Nystrom stages (nystrom.hip, nystrom_bwd.hip),
// the Linear / LayerNorm backward blocks and the PPEG stencil (peg.hip):
//   * the adjoint of the sequence assembly [cls | h | wrap] with _fc1's dropout mask and activation derivative folded in;
//   * the head on ONE row (mask + residual, the last LayerNorm, _fc2) and its backward;
//   * the cls-row tail of layer 2: after layer 2 only row 0 is read, so softmax(q kl^T) wz + conv(v) and to_out are needed for
//     one query row, and their adjoints are one row of d_q, a stencil's reach of d_v, and dense d_kl / d_wz.
// Exact fp32 on the VALU (everything here is one row or one pass over memory), no atomics, every sum in a fixed order: two runs
// give the same bits.  Blocks are 256 threads = 4 waves.
#include "internal.h"

namespace {

constexpr int RM = 256;   // landmarks
constexpr int RD = 64;    // head dim

// d act(x) / dx, the formulas of ln_bwd.hip's activation pass; RRT_ACT_NONE: 1
__device__ __forceinline__ float act_grad(float x, int act) {
  if (act == RRT_ACT_GELU) return 0.5f * (1.0f + erff(x * 0.70710678118654752f)) + x * 0.3989422804014327f * __expf(-0.5f * x * x);
  if (act == RRT_ACT_RELU) return x > 0.f ? 1.0f : 0.f;
  return 1.0f;
}

// the block's total of v, the same value in every thread: wave totals, then the four of them in a fixed order
__device__ __forceinline__ float block_sum(float v, float* red4) {
  v = wave_sum(v);
  __syncthreads();                       // the previous total has been read
  if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red4[0] + red4[1]) + (red4[2] + red4[3]);
}

// ---- assemble adjoint: seq = [cls | h_0 .. h_{N-1} | h_0 .. h_{wrap-1}], h = drop(act(hpre))
//   d_cls = d_seq[0] ; d_hpre[i] = (d_seq[1 + i] + (i < wrap ? d_seq[1 + N + i] : 0)) * mask[i] * act'(hpre[i])
// A wave per row in turn (row N stands for the cls row), whole float4s.  hpre may be null when act is RRT_ACT_NONE.
__global__ __launch_bounds__(256) void transmil_assemble_bwd_kernel(const float* __restrict__ d_seq, const float* __restrict__ hpre,
                                                                    float* __restrict__ d_emb, float* __restrict__ d_cls, int N,
                                                                    int wrap, int dim, int act, unsigned thresh, unsigned seed,
                                                                    float scale) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r = blockIdx.x * 4 + wave; r <= N; r += gridDim.x * 4) {
    if (r == N) {
      for (int c = lane * 4; c < dim; c += 256) *(float4*)(d_cls + c) = *(const float4*)(d_seq + c);
      continue;
    }
    const float* a = d_seq + (size_t)(1 + r) * dim;
    const float* b = d_seq + (size_t)(1 + N + r) * dim;
    const size_t row0 = (size_t)r * dim;
    for (int c = lane * 4; c < dim; c += 256) {
      float4 g = *(const float4*)(a + c);
      if (r < wrap) {
        const float4 o = *(const float4*)(b + c);
        g.x += o.x; g.y += o.y; g.z += o.z; g.w += o.w;
      }
      if (thresh) {
        const unsigned long long i = row0 + c;
        g.x = rrt_drop_keep(seed, i, thresh) ? g.x * scale : 0.f;
        g.y = rrt_drop_keep(seed, i + 1, thresh) ? g.y * scale : 0.f;
        g.z = rrt_drop_keep(seed, i + 2, thresh) ? g.z * scale : 0.f;
        g.w = rrt_drop_keep(seed, i + 3, thresh) ? g.w * scale : 0.f;
      }
      if (act != RRT_ACT_NONE) {
        const float4 x = *(const float4*)(hpre + row0 + c);
        g.x *= act_grad(x.x, act); g.y *= act_grad(x.y, act); g.z *= act_grad(x.z, act); g.w *= act_grad(x.w, act);
      }
      *(float4*)(d_emb + row0 + c) = g;
    }
  }
}

// ---- y [n_out] = W [n_out, n_in] x + b: a wave per output (n_in % 4 == 0)
__global__ __launch_bounds__(256) void row_linear_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ b, float* __restrict__ y, int n_out, int n_in) {
  const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= n_out) return;
  const float* wr = w + (size_t)j * n_in;
  float s = 0.f;
  for (int i = lane * 4; i < n_in; i += 256) {
    const float4 a = *(const float4*)(x + i), c = *(const float4*)(wr + i);
    s += (a.x * c.x + a.y * c.y) + (a.z * c.z + a.w * c.w);
  }
  s = wave_sum(s);
  if (lane == 0) y[j] = s + (b ? b[j] : 0.f);
}

// ---- its adjoint: d_w [n_out, n_in] = dy (x) x, d_b = dy, d_x = W^T dy.  Block = 64 input columns (n_in % 64 == 0); the four
// waves take the output rows j = wave, wave + 4, ..: a wave reads and writes whole 256-byte lines
__global__ __launch_bounds__(256) void row_linear_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                             const float* __restrict__ w, float* __restrict__ d_w,
                                                             float* __restrict__ d_b, float* __restrict__ d_x, int n_out, int n_in) {
  __shared__ float red[3][64];
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6, i = blockIdx.x * 64 + c;
  const float xi = x[i];
  float acc = 0.f;
  for (int j = g; j < n_out; j += 4) {
    const float d = dy[j];
    acc += d * w[(size_t)j * n_in + i];
    d_w[(size_t)j * n_in + i] = d * xi;
  }
  if (g > 0) red[g - 1][c] = acc;
  __syncthreads();
  if (g == 0) d_x[i] = (acc + red[0][c]) + (red[1][c] + red[2][c]);
  if (blockIdx.x == 0)
    for (int j = threadIdx.x; j < n_out; j += 256) d_b[j] = dy[j];
}

// ---- the head on one row (dim <= 1024, n_classes <= 64), one block:
//   hrow = res + drop(y) ; ln = LayerNorm(hrow) ; logits = W ln + b.  hrow [dim] and stats = (mean, rstd) are kept for the backward.
__global__ __launch_bounds__(256) void transmil_row_head_kernel(const float* __restrict__ res, const float* __restrict__ y,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                const float* __restrict__ w, const float* __restrict__ b,
                                                                float* __restrict__ hrow, float* __restrict__ stats,
                                                                float* __restrict__ logits, int dim, int n_classes,
                                                                unsigned thresh, unsigned seed, float scale) {
  __shared__ float ln[1024];
  __shared__ float red4[4];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  float v[4];
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = t + 256 * k;
    v[k] = 0.f;
    if (i < dim) {
      float yy = y[i];
      if (thresh) yy = rrt_drop_keep(seed, (unsigned long long)i, thresh) ? yy * scale : 0.f;
      v[k] = res[i] + yy;
      hrow[i] = v[k];
      s += v[k];
    }
  }
  const float inv_d = 1.0f / (float)dim;
  const float mean = block_sum(s, red4) * inv_d;
  float sq = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (t + 256 * k < dim) {
      v[k] -= mean;
      sq += v[k] * v[k];
    }
  const float rstd = 1.0f / sqrtf(block_sum(sq, red4) * inv_d + LN_EPS);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = t + 256 * k;
    if (i < dim) ln[i] = v[k] * rstd * gamma[i] + beta[i];
  }
  if (t == 0) {
    stats[0] = mean;
    stats[1] = rstd;
  }
  __syncthreads();
  for (int c = wv; c < n_classes; c += 4) {
    float a = 0.f;
    for (int i = lane; i < dim; i += 64) a += ln[i] * w[(size_t)c * dim + i];
    a = wave_sum(a);
    if (lane == 0) logits[c] = a + (b ? b[c] : 0.f);
  }
}

// ---- ... and its backward: d_logits -> d_w [n_classes, dim], d_b, d_gamma, d_beta, d_hrow (the residual's cotangent) and
// d_y = the same row under the forward's mask (the cotangent of layer 2's attention output, zero in every other row)
__global__ __launch_bounds__(256) void transmil_row_head_bwd_kernel(const float* __restrict__ d_logits, const float* __restrict__ hrow,
                                                                    const float* __restrict__ stats, const float* __restrict__ gamma,
                                                                    const float* __restrict__ beta, const float* __restrict__ w,
                                                                    float* __restrict__ d_w, float* __restrict__ d_b,
                                                                    float* __restrict__ d_gamma, float* __restrict__ d_beta,
                                                                    float* __restrict__ d_hrow, float* __restrict__ d_y, int dim,
                                                                    int n_classes, unsigned thresh, unsigned seed, float scale) {
  __shared__ float dl[64];
  __shared__ float red4[4];
  const int t = threadIdx.x;
  if (t < n_classes) {
    dl[t] = d_logits[t];
    d_b[t] = dl[t];
  }
  __syncthreads();
  const float mean = stats[0], rstd = stats[1];
  float xh[4], g[4];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = t + 256 * k;
    xh[k] = g[k] = 0.f;
    if (i < dim) {
      xh[k] = (hrow[i] - mean) * rstd;
      const float lnv = xh[k] * gamma[i] + beta[i];
      float dln = 0.f;
      for (int c = 0; c < n_classes; ++c) {
        dln += dl[c] * w[(size_t)c * dim + i];
        d_w[(size_t)c * dim + i] = dl[c] * lnv;
      }
      d_gamma[i] = dln * xh[k];
      d_beta[i] = dln;
      g[k] = dln * gamma[i];
      s1 += g[k];
      s2 += g[k] * xh[k];
    }
  }
  const float inv_d = 1.0f / (float)dim;
  const float c1 = block_sum(s1, red4) * inv_d;
  const float c2 = block_sum(s2, red4) * inv_d;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = t + 256 * k;
    if (i < dim) {
      const float dh = rstd * (g[k] - c1 - xh[k] * c2);
      d_hrow[i] = dh;
      d_y[i] = thresh ? (rrt_drop_keep(seed, (unsigned long long)i, thresh) ? dh * scale : 0.f) : dh;
    }
  }
}

// a1 [256] = softmax(q[row] kl^T) of head h into LDS, thread = landmark (the arithmetic of nystrom_row.hip's nys_row_r_kernel);
// qs [64] receives the query row.  Ends with a barrier.
__device__ __forceinline__ void row_softmax(const float* __restrict__ qkv, const float* __restrict__ kl, long row, int h, int hd,
                                            float* qs, float* red, float* a1) {
  const int t = threadIdx.x;
  if (t < RD) qs[t] = qkv[(size_t)row * 3 * hd + (size_t)h * RD + t];
  __syncthreads();
  const float* kr = kl + ((size_t)h * RM + t) * RD;
  float s = 0.f;
  for (int c = 0; c < RD; c += 4) {
    const float4 kv = *(const float4*)(kr + c);
    s += qs[c] * kv.x;
    s += qs[c + 1] * kv.y;
    s += qs[c + 2] * kv.z;
    s += qs[c + 3] * kv.w;
  }
  red[t] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) red[t] = fmaxf(red[t], red[t + o]);
    __syncthreads();
  }
  const float e = expf(s - red[0]);
  __syncthreads();
  red[t] = e;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  a1[t] = e / red[0];
  __syncthreads();
}

// ---- o_row [heads * 64] = softmax(q[row] kl^T) wz + sum_tap conv_w[h, tap] v[row + tap - ks / 2] (rows outside [0, np) are
// zero): block = head; thread (g, c) sums landmarks 64 g .. 64 g + 63 and the taps g, g + 4, .. of column c, the four
// partials are added in a fixed order
__global__ __launch_bounds__(256) void nys_out_row_kernel(const float* __restrict__ qkv, const float* __restrict__ kl,
                                                          const float* __restrict__ wz, const float* __restrict__ conv_w,
                                                          float* __restrict__ o_row, long row, long np, int heads, int ks) {
  __shared__ __attribute__((aligned(16))) float qs[RD];
  __shared__ float red[RM];
  __shared__ float a1[RM];
  __shared__ float part[3][RD];
  const int h = blockIdx.x, t = threadIdx.x, c = t & 63, g = t >> 6, hd = heads * RD;
  row_softmax(qkv, kl, row, h, hd, qs, red, a1);
  const float* wp = wz + ((size_t)h * RM + g * 64) * RD + c;
  float acc = 0.f;
  for (int i = 0; i < 64; ++i) acc += a1[g * 64 + i] * wp[(size_t)i * RD];
  if (conv_w) {
    const int half = ks >> 1;
    for (int tap = g; tap < ks; tap += 4) {
      const long r2 = row + tap - half;
      if (r2 >= 0 && r2 < np) acc += conv_w[(size_t)h * ks + tap] * qkv[(size_t)r2 * 3 * hd + 2 * hd + (size_t)h * RD + c];
    }
  }
  if (g > 0) part[g - 1][c] = acc;
  __syncthreads();
  if (g == 0) o_row[(size_t)h * RD + c] = (acc + part[0][c]) + (part[1][c] + part[2][c]);
}

// ---- its adjoint under d_o_row [heads * 64]; d_qkv has been zeroed by the launcher.  Block = head:
//   d_wz[t, c] = a1_t d_o_c ; d_a1_t = d_o . wz[t] ; d_s = a1 (d_a1 - a1 . d_a1) ; d_kl[t, c] = d_s_t q_c ; d_q = d_s^T kl ;
//   d_conv_w[tap] = d_o . v[row + tap - half] ; d_v[row + tap - half] = conv_w[tap] d_o
__global__ __launch_bounds__(256) void nys_out_row_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ kl,
                                                              const float* __restrict__ wz, const float* __restrict__ conv_w,
                                                              const float* __restrict__ d_o_row, float* __restrict__ d_qkv,
                                                              float* __restrict__ d_kl, float* __restrict__ d_wz,
                                                              float* __restrict__ d_conv_w, long row, long np, int heads, int ks) {
  __shared__ __attribute__((aligned(16))) float qs[RD];
  __shared__ __attribute__((aligned(16))) float dos[RD];
  __shared__ float red[RM];
  __shared__ float a1[RM];
  __shared__ float ds[RM];
  __shared__ float part[3][RD];
  const int h = blockIdx.x, t = threadIdx.x, c = t & 63, g = t >> 6, hd = heads * RD;
  if (t < RD) dos[t] = d_o_row[(size_t)h * RD + t];
  row_softmax(qkv, kl, row, h, hd, qs, red, a1);      // (its barriers publish dos as well)
  const float* wr = wz + ((size_t)h * RM + t) * RD;
  float da = 0.f;
  for (int k = 0; k < RD; k += 4) {
    const float4 wv = *(const float4*)(wr + k);
    da += dos[k] * wv.x;
    da += dos[k + 1] * wv.y;
    da += dos[k + 2] * wv.z;
    da += dos[k + 3] * wv.w;
  }
  red[t] = a1[t] * da;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  ds[t] = a1[t] * (da - red[0]);
  __syncthreads();
  float* dwz_h = d_wz + (size_t)h * RM * RD;
  float* dkl_h = d_kl + (size_t)h * RM * RD;
  for (int idx = t; idx < RM * RD; idx += 256) {
    const int tt = idx >> 6, cc = idx & 63;
    dwz_h[idx] = a1[tt] * dos[cc];
    dkl_h[idx] = ds[tt] * qs[cc];
  }
  const float* kp = kl + ((size_t)h * RM + g * 64) * RD + c;
  float acc = 0.f;
  for (int i = 0; i < 64; ++i) acc += ds[g * 64 + i] * kp[(size_t)i * RD];
  if (g > 0) part[g - 1][c] = acc;
  __syncthreads();
  if (g == 0) d_qkv[(size_t)row * 3 * hd + (size_t)h * RD + c] = (acc + part[0][c]) + (part[1][c] + part[2][c]);
  if (conv_w) {
    const int half = ks >> 1;
    if (t < ks) {
      const long r2 = row + t - half;
      float s = 0.f;
      if (r2 >= 0 && r2 < np) {
        const float* vp = qkv + (size_t)r2 * 3 * hd + 2 * hd + (size_t)h * RD;
        for (int k = 0; k < RD; ++k) s += dos[k] * vp[k];
      }
      d_conv_w[(size_t)h * ks + t] = s;
    }
    for (int idx = t; idx < ks * RD; idx += 256) {
      const int tap = idx >> 6, cc = idx & 63;
      const long r2 = row + tap - half;
      if (r2 >= 0 && r2 < np) d_qkv[(size_t)r2 * 3 * hd + 2 * hd + (size_t)h * RD + cc] = conv_w[(size_t)h * ks + tap] * dos[cc];
    }
  }
}

}  // namespace

hipError_t launch_transmil_assemble_backward(const float* d_seq, const float* hpre, float* d_emb, float* d_cls, int N, int side,
                                             int dim, int act, unsigned thresh, unsigned seed, float scale, hipStream_t st) {
  const int need = (N + 1 + 3) / 4;
  transmil_assemble_bwd_kernel<<<dim3(need < 2048 ? need : 2048), 256, 0, st>>>(d_seq, hpre, d_emb, d_cls, N, side * side - N, dim,
                                                                               act, thresh, seed, scale);
  return hipGetLastError();
}

hipError_t launch_row_linear(const float* x, const float* w, const float* b, float* y, int n_out, int n_in, hipStream_t st) {
  row_linear_kernel<<<dim3((n_out + 3) / 4), 256, 0, st>>>(x, w, b, y, n_out, n_in);
  return hipGetLastError();
}

hipError_t launch_row_linear_backward(const float* dy, const float* x, const float* w, float* d_w, float* d_b, float* d_x,
                                      int n_out, int n_in, hipStream_t st) {
  if (n_in % 64) return hipErrorInvalidValue;
  row_linear_bwd_kernel<<<dim3(n_in / 64), 256, 0, st>>>(dy, x, w, d_w, d_b, d_x, n_out, n_in);
  return hipGetLastError();
}

hipError_t launch_transmil_row_head(const float* res, const float* y, const float* gamma, const float* beta, const float* w,
                                    const float* b, float* hrow, float* stats, float* logits, int dim, int n_classes,
                                    unsigned thresh, unsigned seed, float scale, hipStream_t st) {
  if (dim > 1024 || n_classes > 64) return hipErrorInvalidValue;
  transmil_row_head_kernel<<<1, 256, 0, st>>>(res, y, gamma, beta, w, b, hrow, stats, logits, dim, n_classes, thresh, seed, scale);
  return hipGetLastError();
}

hipError_t launch_transmil_row_head_backward(const float* d_logits, const float* hrow, const float* stats, const float* gamma,
                                             const float* beta, const float* w, float* d_w, float* d_b, float* d_gamma,
                                             float* d_beta, float* d_hrow, float* d_y, int dim, int n_classes, unsigned thresh,
                                             unsigned seed, float scale, hipStream_t st) {
  if (dim > 1024 || n_classes > 64) return hipErrorInvalidValue;
  transmil_row_head_bwd_kernel<<<1, 256, 0, st>>>(d_logits, hrow, stats, gamma, beta, w, d_w, d_b, d_gamma, d_beta, d_hrow, d_y,
                                                  dim, n_classes, thresh, seed, scale);
  return hipGetLastError();
}

hipError_t launch_nystrom_output_row(const float* qkv, const float* kl, const float* wz, const float* conv_w, float* o_row,
                                     long row, long np, int heads, int ks, hipStream_t st) {
  if (row < 0 || row >= np) return hipErrorInvalidValue;
  nys_out_row_kernel<<<heads, 256, 0, st>>>(qkv, kl, wz, conv_w, o_row, row, np, heads, ks);
  return hipGetLastError();
}

hipError_t launch_nystrom_output_row_backward(const float* qkv, const float* kl, const float* wz, const float* conv_w,
                                              const float* d_o_row, float* d_qkv, float* d_kl, float* d_wz, float* d_conv_w,
                                              long row, long np, int heads, int ks, hipStream_t st) {
  if (row < 0 || row >= np) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(d_qkv, 0, (size_t)np * 3 * heads * RD * sizeof(float), st);
  if (e != hipSuccess) return e;
  nys_out_row_bwd_kernel<<<heads, 256, 0, st>>>(qkv, kl, wz, conv_w, d_o_row, d_qkv, d_kl, d_wz, d_conv_w, row, np, heads, ks);
  return hipGetLastError();
}
