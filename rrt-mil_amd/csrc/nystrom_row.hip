// nystrom_row.hip -- one query row of the Nystrom-approximated attention matrix (modules/nystrom_attention.py:143-147, the
// return_attn branch): the slide-level heat map of TransMIL is the class token's row.  Exact fp32, the score tile on
// v_mfma_f32_16x16x4_f32, no atomics, every sum in a fixed order: the same inputs give the same bits.
//
// Per head, from what the forward leaves in its workspace (layouts of nystrom.hip):
//   a1      = softmax(q[row] kl^T)                          [256]
//   r       = a1 z                                          [256]       nys_row_r_kernel
//   attn[j] = sum_i r_i exp(ql_i . k_j - lse3_i)            j < np      nys_row_keys_kernel
// lse3 [heads, 256] is the row log-sum-exp of ql k^T over ALL np keys (the optional output of the landmark attention's merge),
// so softmax(ql k^T) [256, np] is never written: a block recomputes its 64 x 256 tile of it on the matrix cores.
// The pad keys keep their share, entries may be negative (r is not a probability vector), the exponent is <= 0 up to rounding.
#include "nystrom_tiles.h"

namespace {

// ---- r = softmax(q[row] kl^T) z : block = head, thread = landmark (a score, then a column of z)
__global__ __launch_bounds__(256) void nys_row_r_kernel(const float* __restrict__ qkv, const float* __restrict__ kl,
                                                        const float* __restrict__ z, float* __restrict__ r, long row, int heads) {
  __shared__ __attribute__((aligned(16))) float qs[ND];
  __shared__ float red[NM];
  __shared__ float a1[NM];
  const int h = blockIdx.x, t = threadIdx.x, hd = heads * ND;
  if (t < ND) qs[t] = qkv[(size_t)row * 3 * hd + (size_t)h * ND + t];
  __syncthreads();
  const float* kr = kl + ((size_t)h * NM + t) * ND;
  float s = 0.f;
  for (int c = 0; c < ND; c += 4) {
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
  const float* zc = z + (size_t)h * NM * NM + t;          // column t of z: the 256 threads read one line of z per step
  float acc = 0.f;
  for (int i = 0; i < NM; ++i) acc += a1[i] * zc[(size_t)i * NM];
  r[(size_t)h * NM + t] = acc;
}

// ---- attn[h, key - col0] = sum_i r_i exp(ql_i . k_key - lse3_i) : block (64-key tile, head).  The sibling of
// scores_softmax_256: the keys are the rows, ql takes the place of kl and goes through LDS in 64-landmark pieces; a piece's
// scores are folded into the row sums at once (a lane's own four accumulators in column order, piece after piece, then the
// 16 lanes of the row).  Keys below col0 (the front pad of a whole call) are computed and not stored.
__global__ __launch_bounds__(256) void nys_row_keys_kernel(const float* __restrict__ qkv, const float* __restrict__ ql,
                                                           const float* __restrict__ lse3, const float* __restrict__ r,
                                                           float* __restrict__ attn, long col0, long out_ld, int heads) {
  __shared__ __attribute__((aligned(16))) float As[64 * LDA];
  __shared__ __attribute__((aligned(16))) float Bs[64 * LDB];
  const int h = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6, hd = heads * ND;
  const long t0 = (long)blockIdx.x * 64;
  const size_t ld3 = (size_t)3 * hd;
  stage_rows(As, LDA, qkv + (size_t)t0 * ld3 + hd + (size_t)h * ND, ld3, 64);
  const float* ql_h = ql + (size_t)h * NM * ND;
  const float* r_h = r + (size_t)h * NM + (lane & 15);
  const float* l_h = lse3 + (size_t)h * NM + (lane & 15);
  float sum[4] = {0.f, 0.f, 0.f, 0.f};
  for (int ct = 0; ct < 4; ++ct) {
    __syncthreads();                       // the previous piece's reads of Bs are done (and, first, As is staged)
    stage_64x64_t(Bs, LDB, ql_h + (size_t)ct * 64 * ND, ND);
    __syncthreads();
    f32x4 s[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    mma_16x64(As + w * 16 * LDA, LDA, Bs, LDB, ND, s);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float ri = r_h[64 * ct + 16 * j], li = l_h[64 * ct + 16 * j];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) sum[rr] += ri * expf(s[j][rr] - li);
    }
  }
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const float v = row16_sum(sum[rr]);
    const long key = t0 + 16 * w + 4 * (lane >> 4) + rr;
    if ((lane & 15) == 0 && key >= col0) attn[(size_t)h * out_ld + (key - col0)] = v;
  }
}

}  // namespace

// r [heads, 256], attn [heads, out_ld]: columns col0 .. np - 1 of the row (out_ld >= np - col0)
hipError_t launch_nystrom_attn_row(const float* qkv, const float* ql, const float* kl, const float* z, const float* lse3,
                                   float* r, float* attn, long row_padded, long np, long col0, long out_ld, int heads,
                                   hipStream_t st) {
  nys_row_r_kernel<<<heads, 256, 0, st>>>(qkv, kl, z, r, row_padded, heads);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  nys_row_keys_kernel<<<dim3((unsigned)(np / 64), heads), 256, 0, st>>>(qkv, ql, lse3, r, attn, col0, out_ld, heads);
  return hipGetLastError();
}
