// nystrom_bwd.hip -- the backward of Nystrom attention (nystrom.hip), for training the TransMIL baseline.  Exact fp32; every
// matrix product runs on v_mfma_f32_16x16x4_f32.  No atomics, every sum has a fixed order: the same inputs give the same bits.
//
// Forward, per head (m = 256 landmarks, d = 64, np = 256 l rows, q scaled):
//   A1 = softmax(q kl^T)   A2 = softmax(ql kl^T)   A3 = softmax(ql k^T)   AV = A3 v   Z = pinv(A2)   W = Z AV
//   O = A1 W + conv(v)
// Reverse, given dO:
//   output     dW = A1^T dO, dS1 = A1 (dO W^T - rowsum(A1 . dO W^T)), dq = dS1 kl, dkl = dS1^T q, dv = conv^T(dO),
//              dconv_w[tap] = sum dO[t] . v[t + tap - half].  A1 is recomputed per 64-token tile; a block walks the tiles of
//              one chunk and leaves one partial record of dW | dkl | dconv_w, the records are merged in chunk order.
//   zav        dZ = dW AV^T, dAV = Z^T dW
//   lattn      P = exp(ql k^T - lse3), dv += P^T dAV, dS3 = P (dAV v^T - rowsum(dAV . AV)), dk = dS3^T ql, dql = dS3 k (chunked
//              partials as above).  A block per (chunk of 64-key tiles, head) walks all 256 landmarks: every dk / dv row is
//              written exactly once.
//   pinv_sim   the reverse of the iteration z <- 1/4 z (13 I - xz (15 I - xz (7 I - xz))), xz = A2 z, with every iterate
//              recomputed from A2 (and the tangent along the scale of z0 carried forward, for the gradient through den);
//              then z0 = A2^T / den, den = (largest row sum) (largest column sum) over ALL heads: the
//              gradient through the largest column sum goes to every entry of the columns that attain it (shared evenly among
//              columns whose sums are equal bit for bit, torch's rule); the part through the largest row sum vanishes behind
//              the softmax backward (a row of a softmax sums to one) and is left out; then the softmax backward of A2 and
//              dql += dS2 kl, dkl += dS2^T ql.
//   landmarks  row t of landmark j receives dql[j] / l in its q columns and dkl[j] / l in its k columns
//
// b sequences per launch (the trailing `b` of every launcher, 1 = the single-sequence launches, bit for bit): the item is
// blockIdx.z of the tile kernels and rides in the head index (item * heads + head) of everything laid out per head, so each
// item's stencil, pad rows and chunk records are its own.  den stays ONE scalar over all b * heads matrices; dconv_w is summed
// over the items in item order.
#include "nystrom_tiles.h"

namespace {

constexpr int TILE_LDS_FLOATS = 64 * LDA + 64 * LDB + 64 * LDA;          // Abuf | Bbuf | Pbuf ; the stencil reuses all of it

// ---- batched GEMM C = s (op(A) op(B)) + t I (+ C when acc), optionally C2 = s2 (op(A) op(B)) + t2 I.  op = transpose when
// TA / TB: A is then stored [K, M], B [N, K].  M a multiple of 64, N and K of 32.  block (N / 32, M / 64, batch), a 64 x 32
// tile; the k-steps run in order, so the sum's order is fixed.
struct GemmArgs {
  const float *A, *B;
  float *C, *C2;
  int K, lda, ldb, ldc;
  size_t sA, sB, sC;
  float s, t, s2, t2;
  int acc;
};
constexpr int GK = 32, GN = 32, GLDA = 36, GLDB = 48;
template <bool TA, bool TB>
__global__ __launch_bounds__(256) void nysb_gemm_kernel(const GemmArgs p) {
  __shared__ __attribute__((aligned(16))) float As[64 * GLDA];
  __shared__ __attribute__((aligned(16))) float Bs[GK * GLDB];
  const int b = blockIdx.z, m0 = blockIdx.y * 64, n0 = blockIdx.x * GN, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float* A = p.A + b * p.sA;
  const float* B = p.B + b * p.sB;
  f32x4 acc[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < p.K; k0 += GK) {
    __syncthreads();
    if (!TA) {
      const int ar = tid >> 3, ac = (tid & 7) * 4;
      *(float4*)(As + ar * GLDA + ac) = *(const float4*)(A + (size_t)(m0 + ar) * p.lda + k0 + ac);
      *(float4*)(As + (ar + 32) * GLDA + ac) = *(const float4*)(A + (size_t)(m0 + ar + 32) * p.lda + k0 + ac);
    } else {
#pragma unroll
      for (int i = tid; i < 512; i += 256) {
        const int kr = i >> 4, mc = (i & 15) * 4;
        const float4 v = *(const float4*)(A + (size_t)(k0 + kr) * p.lda + m0 + mc);
        As[(mc + 0) * GLDA + kr] = v.x;
        As[(mc + 1) * GLDA + kr] = v.y;
        As[(mc + 2) * GLDA + kr] = v.z;
        As[(mc + 3) * GLDA + kr] = v.w;
      }
    }
    if (!TB) {
      const int br = tid >> 3, bc = (tid & 7) * 4;
      *(float4*)(Bs + br * GLDB + bc) = *(const float4*)(B + (size_t)(k0 + br) * p.ldb + n0 + bc);
    } else {
      const int nr = tid >> 3, kc = (tid & 7) * 4;
      const float4 v = *(const float4*)(B + (size_t)(n0 + nr) * p.ldb + k0 + kc);
      Bs[(kc + 0) * GLDB + nr] = v.x;
      Bs[(kc + 1) * GLDB + nr] = v.y;
      Bs[(kc + 2) * GLDB + nr] = v.z;
      Bs[(kc + 3) * GLDB + nr] = v.w;
    }
    __syncthreads();
    mma_16x64<2>(As + w * 16 * GLDA, GLDA, Bs, GLDB, GK, acc);
  }
  const int row0 = m0 + 16 * w + 4 * (lane >> 4);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = n0 + 16 * j + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = row0 + r;
      const float d = row == col ? 1.f : 0.f;
      const size_t o = b * p.sC + (size_t)row * p.ldc + col;
      float v = p.s * acc[j][r] + p.t * d;
      if (p.acc) v += p.C[o];
      p.C[o] = v;
      if (p.C2) p.C2[o] = p.s2 * acc[j][r] + p.t2 * d;
    }
  }
}

// C [batch, M, N] = s op(A) op(B) + t I (+ C); all matrices dense row-major as stored
hipError_t gemm(bool ta, bool tb, const float* A, const float* B, float* C, float* C2, int M, int N, int K, int batch, float s,
                float t, float s2, float t2, int acc, hipStream_t st) {
  GemmArgs p{A, B, C, C2, K, ta ? M : K, tb ? K : N, N, (size_t)M * K, (size_t)K * N, (size_t)M * N, s, t, s2, t2, acc};
  const dim3 grid(N / GN, M / 64, batch);
  if (ta) nysb_gemm_kernel<true, false><<<grid, 256, 0, st>>>(p);
  else if (tb) nysb_gemm_kernel<false, true><<<grid, 256, 0, st>>>(p);
  else nysb_gemm_kernel<false, false><<<grid, 256, 0, st>>>(p);
  return hipGetLastError();
}

// a tile of accumulators into LDS as an A operand: natural dst[row][16 j + col], transposed dst[16 j + col][row]
__device__ __forceinline__ void put_tile(float* dst, const f32x4 (&v)[4]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int j = 0; j < 4; ++j) dst[(16 * w + 4 * (lane >> 4) + r) * LDA + 16 * j + (lane & 15)] = v[j][r];
}
__device__ __forceinline__ void put_tile_t(float* dst, const f32x4 (&v)[4]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int j = 0; j < 4; ++j) dst[(16 * j + (lane & 15)) * LDA + 16 * w + 4 * (lane >> 4) + r] = v[j][r];
}

// a [256, 64] record of this block: acc[ct] holds rows 64 ct + 16 w + 4 (lane >> 4) + r, columns 16 j + (lane & 15)
__device__ __forceinline__ void store_record(float* __restrict__ rec, const f32x4 (&acc)[4][4]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        rec[(size_t)(64 * ct + 16 * w + 4 * (lane >> 4) + r) * ND + 16 * j + (lane & 15)] = acc[ct][j][r];
}

// ---- output backward: block (chunk of 64-token tiles, head, item)
__global__ __launch_bounds__(256) void nysb_output_kernel(const float* __restrict__ qkv, const float* __restrict__ kl,
                                                          const float* __restrict__ wz, const float* __restrict__ conv_w,
                                                          const float* __restrict__ d_o, float* __restrict__ d_qkv,
                                                          float* __restrict__ pW, float* __restrict__ pK, float* __restrict__ pC,
                                                          int np, int heads, int ks, int nsub, int sub_per_chunk) {
  __shared__ __attribute__((aligned(16))) float lds[TILE_LDS_FLOATS];
  float* Abuf = lds;
  float* Bbuf = lds + 64 * LDA;
  float* Pbuf = Bbuf + 64 * LDB;
  const int ch = blockIdx.x, h = blockIdx.y, nch = gridDim.x, hd = heads * ND;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const size_t ld3 = (size_t)3 * hd, bh = (size_t)blockIdx.z * heads + h;
  qkv += (size_t)blockIdx.z * np * ld3;    // this item's own padded sequence: the stencil's taps stay inside [0, np)
  d_qkv += (size_t)blockIdx.z * np * ld3;
  d_o += (size_t)blockIdx.z * np * hd;
  const float* kl_h = kl + bh * NM * ND;
  const float* wz_h = wz + bh * NM * ND;
  const int s_begin = ch * sub_per_chunk, s_end = min(nsub, s_begin + sub_per_chunk);
  f32x4 accW[4][4], accK[4][4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int j = 0; j < 4; ++j) accW[ct][j] = accK[ct][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float cacc = 0.f;                       // lane tap of wave w: this wave's share of dconv_w[tap]
  for (int sc = s_begin; sc < s_end; ++sc) {
    const int t0 = sc * 64;
    const float* qrow = qkv + (size_t)t0 * ld3 + (size_t)h * ND;
    const float* dorow = d_o + (size_t)t0 * hd + (size_t)h * ND;
    __syncthreads();                       // the previous tile's reads of the LDS are done
    stage_rows(Abuf, LDA, qrow, ld3, 64);
    f32x4 s[4][4], dp[4][4];
    scores_softmax_256(Abuf, Bbuf, kl_h, s);
    // dp = dO W^T
    __syncthreads();
    stage_rows(Abuf, LDA, dorow, hd, 64);
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      __syncthreads();
      stage_64x64_t(Bbuf, LDB, wz_h + (size_t)ct * 64 * ND, ND);
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 4; ++j) dp[ct][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      mma_16x64(Abuf + w * 16 * LDA, LDA, Bbuf, LDB, ND, dp[ct]);
    }
    // dS1 = A1 (dp - rowsum(A1 dp))
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float d1 = 0.f;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int j = 0; j < 4; ++j) d1 += s[ct][j][r] * dp[ct][j][r];
      d1 = row16_sum(d1);
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int j = 0; j < 4; ++j) dp[ct][j][r] = s[ct][j][r] * (dp[ct][j][r] - d1);
    }
    // dW += A1^T dO
    __syncthreads();
    stage_rows(Bbuf, LDB, dorow, hd, 64);
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      __syncthreads();
      put_tile_t(Pbuf, s[ct]);
      __syncthreads();
      mma_16x64(Pbuf + w * 16 * LDA, LDA, Bbuf, LDB, 64, accW[ct]);
    }
    // dkl += dS1^T q
    __syncthreads();
    stage_rows(Bbuf, LDB, qrow, ld3, 64);
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      __syncthreads();
      put_tile_t(Pbuf, dp[ct]);
      __syncthreads();
      mma_16x64(Pbuf + w * 16 * LDA, LDA, Bbuf, LDB, 64, accK[ct]);
    }
    // dq = dS1 kl
    f32x4 dq[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) dq[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      __syncthreads();
      put_tile(Pbuf, dp[ct]);
      stage_rows(Bbuf, LDB, kl_h + (size_t)ct * 64 * ND, ND, 64);
      __syncthreads();
      mma_16x64(Pbuf + w * 16 * LDA, LDA, Bbuf, LDB, 64, dq);
    }
    float* dst = d_qkv + (size_t)(t0 + 16 * w + 4 * (lane >> 4)) * ld3 + (size_t)h * ND + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        dst[(size_t)r * ld3 + 16 * j] = dq[j][r];
        dst[(size_t)r * ld3 + hd + 16 * j] = 0.f;                       // the k third: filled by the later stages
      }
    if (conv_w) {
      // dv = conv^T(dO): dO rows t0 - half .. t0 + 63 + half of this head (zero outside the padded sequence)
      const int half = ks >> 1, rows = 64 + 2 * half;
      float* Xs = lds;
      __syncthreads();
      for (int i = threadIdx.x; i < rows * 16; i += 256) {
        const int r = i >> 4, c = (i & 15) * 4, t = t0 - half + r;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t >= 0 && t < np) v = *(const float4*)(d_o + (size_t)t * hd + (size_t)h * ND + c);
        *(float4*)(Xs + r * 64 + c) = v;
      }
      __syncthreads();
      const float* cw = conv_w + (size_t)h * ks;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * w + 4 * (lane >> 4) + r;
        float c4[4] = {0.f, 0.f, 0.f, 0.f};
        for (int tap = 0; tap < ks; ++tap) {
          const float wt = cw[ks - 1 - tap];                            // the flipped taps
          const float* xp = Xs + (row + tap) * 64 + (lane & 15);
#pragma unroll
          for (int j = 0; j < 4; ++j) c4[j] += wt * xp[16 * j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) dst[(size_t)r * ld3 + 2 * hd + 16 * j] = c4[j];
      }
      // dconv_w[tap] += sum_r sum_c dO[t0 + r][c] v[t0 + r + tap - half][c]: v rows t0 - half .. as above, then the dO tile
      float* Vs = lds;
      float* Ds = lds + 126 * 64;
      __syncthreads();
      for (int i = threadIdx.x; i < rows * 16; i += 256) {
        const int r = i >> 4, c = (i & 15) * 4, t = t0 - half + r;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t >= 0 && t < np) v = *(const float4*)(qkv + (size_t)t * ld3 + 2 * hd + (size_t)h * ND + c);
        *(float4*)(Vs + r * 64 + c) = v;
      }
      for (int i = threadIdx.x; i < 64 * 16; i += 256) {
        const int r = i >> 4, c = (i & 15) * 4;
        *(float4*)(Ds + r * 64 + c) = *(const float4*)(dorow + (size_t)r * hd + c);
      }
      __syncthreads();
      for (int tap = 0; tap < ks; ++tap) {
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) sum += Ds[(16 * w + r) * 64 + lane] * Vs[(16 * w + r + tap) * 64 + lane];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        if (lane == tap) cacc += sum;
      }
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int j = 0; j < 4; ++j) dst[(size_t)r * ld3 + 2 * hd + 16 * j] = 0.f;
    }
  }
  const size_t rec = bh * nch + ch;
  store_record(pW + rec * NM * ND, accW);
  store_record(pK + rec * NM * ND, accK);
  __syncthreads();
  lds[threadIdx.x] = cacc;
  __syncthreads();
  if (threadIdx.x < 64) pC[rec * 64 + threadIdx.x] = ((lds[threadIdx.x] + lds[64 + threadIdx.x]) + lds[128 + threadIdx.x]) + lds[192 + threadIdx.x];
}

// out[h, i] (+)= the sum over the items, in item order, and within an item over the chunks, in chunk order, of
// part[item, h, c, i]; i < out_elems <= elems.  (items = 1 with the grid's y over item * heads + head: a sum per item.)
__global__ __launch_bounds__(256) void nysb_merge_kernel(const float* __restrict__ part, float* __restrict__ out, int nch,
                                                         int elems, int out_elems, int acc, int items) {
  const int h = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= out_elems) return;
  const size_t item_stride = (size_t)gridDim.y * nch * elems;
  float s = 0.f;
  for (int it = 0; it < items; ++it) {
    const float* p = part + it * item_stride + (size_t)h * nch * elems + i;
    for (int c = 0; c < nch; ++c) s += p[(size_t)c * elems];
  }
  float* o = out + (size_t)h * out_elems + i;
  *o = acc ? *o + s : s;
}

// ---- d3[row] = sum_c a[row, c] b[row, c] over 64 columns: a wave per row
__global__ __launch_bounds__(256) void nysb_rowdot_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                          float* __restrict__ d3, int rows) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  float s = a[(size_t)row * ND + lane] * b[(size_t)row * ND + lane];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) d3[row] = s;
}

// ---- landmark attention backward: block (chunk of 64-key tiles, head, item)
__global__ __launch_bounds__(256) void nysb_lattn_kernel(const float* __restrict__ qkv, const float* __restrict__ ql,
                                                         const float* __restrict__ lse, const float* __restrict__ d3,
                                                         const float* __restrict__ d_av, float* __restrict__ d_qkv,
                                                         float* __restrict__ pQ, int heads, int nsub, int sub_per_chunk) {
  __shared__ __attribute__((aligned(16))) float lds[TILE_LDS_FLOATS];
  float* Abuf = lds;
  float* Bbuf = lds + 64 * LDA;
  float* Pbuf = Bbuf + 64 * LDB;
  const int ch = blockIdx.x, h = blockIdx.y, nch = gridDim.x, hd = heads * ND;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const size_t ld3 = (size_t)3 * hd, bh = (size_t)blockIdx.z * heads + h;
  qkv += (size_t)blockIdx.z * nsub * 64 * ld3;
  d_qkv += (size_t)blockIdx.z * nsub * 64 * ld3;
  const float* ql_h = ql + bh * NM * ND;
  const float* dav_h = d_av + bh * NM * ND;
  const int s_begin = ch * sub_per_chunk, s_end = min(nsub, s_begin + sub_per_chunk);
  float lreg[4][4], dreg[4][4];           // of landmark 64 lb + 16 j + (lane & 15)
  f32x4 accQ[4][4];
#pragma unroll
  for (int lb = 0; lb < 4; ++lb)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      lreg[lb][j] = lse[bh * NM + 64 * lb + 16 * j + (lane & 15)];
      dreg[lb][j] = d3[bh * NM + 64 * lb + 16 * j + (lane & 15)];
      accQ[lb][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  for (int sc = s_begin; sc < s_end; ++sc) {
    const float* krow = qkv + (size_t)sc * 64 * ld3 + hd + (size_t)h * ND;
    const float* vrow = krow + hd;
    // T[key][landmark] = k ql^T, G[key][landmark] = v dAV^T
    f32x4 T[4][4], G[4][4];
    __syncthreads();                       // the previous tile's reads of the LDS are done
    stage_rows(Abuf, LDA, krow, ld3, 64);
#pragma unroll
    for (int lb = 0; lb < 4; ++lb) {
      __syncthreads();
      stage_64x64_t(Bbuf, LDB, ql_h + (size_t)lb * 64 * ND, ND);
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 4; ++j) T[lb][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      mma_16x64(Abuf + w * 16 * LDA, LDA, Bbuf, LDB, ND, T[lb]);
    }
    __syncthreads();
    stage_rows(Abuf, LDA, vrow, ld3, 64);
#pragma unroll
    for (int lb = 0; lb < 4; ++lb) {
      __syncthreads();
      stage_64x64_t(Bbuf, LDB, dav_h + (size_t)lb * 64 * ND, ND);
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 4; ++j) G[lb][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      mma_16x64(Abuf + w * 16 * LDA, LDA, Bbuf, LDB, ND, G[lb]);
    }
    // T <- P^T = exp(T - lse), G <- dS3^T = P^T (G - d3)
#pragma unroll
    for (int lb = 0; lb < 4; ++lb)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = expf(T[lb][j][r] - lreg[lb][j]);
          T[lb][j][r] = p;
          G[lb][j][r] = p * (G[lb][j][r] - dreg[lb][j]);
        }
    // dv = P^T dAV, dk = dS3^T ql
    f32x4 dv[4], dk[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) dv[j] = dk[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int lb = 0; lb < 4; ++lb) {
      __syncthreads();
      put_tile(Pbuf, T[lb]);
      stage_rows(Bbuf, LDB, dav_h + (size_t)lb * 64 * ND, ND, 64);
      __syncthreads();
      mma_16x64(Pbuf + w * 16 * LDA, LDA, Bbuf, LDB, 64, dv);
    }
#pragma unroll
    for (int lb = 0; lb < 4; ++lb) {
      __syncthreads();
      put_tile(Pbuf, G[lb]);
      stage_rows(Bbuf, LDB, ql_h + (size_t)lb * 64 * ND, ND, 64);
      __syncthreads();
      mma_16x64(Pbuf + w * 16 * LDA, LDA, Bbuf, LDB, 64, dk);
    }
    // dql += dS3 k
    __syncthreads();
    stage_rows(Bbuf, LDB, krow, ld3, 64);
#pragma unroll
    for (int lb = 0; lb < 4; ++lb) {
      __syncthreads();
      put_tile_t(Pbuf, G[lb]);
      __syncthreads();
      mma_16x64(Pbuf + w * 16 * LDA, LDA, Bbuf, LDB, 64, accQ[lb]);
    }
    float* dst = d_qkv + (size_t)(sc * 64 + 16 * w + 4 * (lane >> 4)) * ld3 + hd + (size_t)h * ND + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        dst[(size_t)r * ld3 + 16 * j] += dk[j][r];
        dst[(size_t)r * ld3 + hd + 16 * j] += dv[j][r];
      }
  }
  store_record(pQ + (bh * nch + ch) * NM * ND, accQ);
}

// ---- pinv backward pieces
// per head and index t: the abs sum of row t and of column t of a2 (the forward's order of summation)
__global__ __launch_bounds__(256) void nysb_sums_kernel(const float* __restrict__ a2, float* __restrict__ rsum,
                                                        float* __restrict__ csum) {
  const int h = blockIdx.x, t = threadIdx.x;
  const float* a = a2 + (size_t)h * NM * NM;
  float rs = 0.f, cs = 0.f;
  for (int i = 0; i < NM; ++i) {
    rs += fabsf(a[(size_t)t * NM + i]);
    cs += fabsf(a[(size_t)i * NM + t]);
  }
  rsum[(size_t)h * NM + t] = rs;
  csum[(size_t)h * NM + t] = cs;
}
// scal = {mr, mc, mr * mc, the number of columns whose sum equals mc} over all heads (of all items): one block
__global__ __launch_bounds__(256) void nysb_scal_kernel(const float* __restrict__ rsum, const float* __restrict__ csum,
                                                        float* __restrict__ scal, int n) {
  __shared__ float red[2][256];
  __shared__ int cnt[256];
  const int t = threadIdx.x;
  float mr = -INFINITY, mc = -INFINITY;
  for (int i = t; i < n; i += 256) {
    mr = fmaxf(mr, rsum[i]);
    mc = fmaxf(mc, csum[i]);
  }
  red[0][t] = mr;
  red[1][t] = mc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
      red[0][t] = fmaxf(red[0][t], red[0][t + o]);
      red[1][t] = fmaxf(red[1][t], red[1][t + o]);
    }
    __syncthreads();
  }
  mr = red[0][0];
  mc = red[1][0];
  int c = 0;
  for (int i = t; i < n; i += 256) c += csum[i] == mc ? 1 : 0;
  cnt[t] = c;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) cnt[t] += cnt[t + o];
    __syncthreads();
  }
  if (t == 0) {
    scal[0] = mr;
    scal[1] = mc;
    scal[2] = mr * mc;
    scal[3] = (float)cnt[0];
  }
}
// z0[i][j] = a2[j][i] / den: block (16 x 16 tile pair, head)
__global__ __launch_bounds__(256) void nysb_z0_kernel(const float* __restrict__ a2, const float* __restrict__ scal,
                                                      float* __restrict__ z) {
  __shared__ float tile[16][17];
  const float denom = scal[2];
  const int h = blockIdx.z, ti = blockIdx.y * 16, tj = blockIdx.x * 16, x = threadIdx.x & 15, y = threadIdx.x >> 4;
  tile[y][x] = a2[((size_t)h * NM + tj + y) * NM + ti + x];
  __syncthreads();
  z[((size_t)h * NM + ti + y) * NM + tj + x] = tile[x][y] / denom;
}
// part[h] = sum over the head's matrix of a . b, in a fixed order
__global__ __launch_bounds__(256) void nysb_dot_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                       float* __restrict__ part) {
  __shared__ float red[256];
  const int h = blockIdx.x, t = threadIdx.x;
  const size_t base = (size_t)h * NM * NM;
  float s = 0.f;
  for (int i = t; i < NM * NM; i += 256) s += a[base + i] * b[base + i];
  red[t] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  if (t == 0) part[h] = red[0];
}
// scal[4] = the sum of the n per-matrix partials in a fixed order: thread t sums partials 64 t .. 64 t + 63 in index order
// (and, beyond 256 * 64 of them, every 256th run of 64 after it), thread 0 adds the runs' sums in run order.  Up to 64
// partials that is the plain sum in index order.
__global__ __launch_bounds__(256) void nysb_tot_kernel(const float* __restrict__ part, float* __restrict__ scal, int n) {
  __shared__ float run[256];
  const int t = threadIdx.x, nrun = (n + 63) / 64;
  float tot = 0.f;
  for (int r0 = 0; r0 < nrun; r0 += 256) {
    float s = 0.f;
    const int beg = (r0 + t) * 64, end = min(n, beg + 64);
    for (int i = beg; i < end; ++i) s += part[i];
    __syncthreads();
    run[t] = s;
    __syncthreads();
    if (t == 0)
      for (int r = 0; r < min(256, nrun - r0); ++r) tot += run[r];
  }
  if (t == 0) scal[4] = tot;
}
// da2[i][j] += dz[j][i] / den + (column (h, j) attains mc ? dden mr / ties : 0), dden = -(sum_h part[h]) / den with
// part[h] = sum(d_z . zd) of matrix h, the tangent of the forward sweep; their sum is scal[4] (nysb_tot_kernel)
__global__ __launch_bounds__(256) void nysb_da2_z0_kernel(float* __restrict__ da2, const float* __restrict__ dz,
                                                          const float* __restrict__ csum, const float* __restrict__ scal) {
  __shared__ float tile[16][17];
  const float mr = scal[0], mc = scal[1], den = scal[2], ties = scal[3], tot = scal[4];
  const float share = (-tot / den) * mr / ties;
  const int h = blockIdx.z, ti = blockIdx.y * 16, tj = blockIdx.x * 16, x = threadIdx.x & 15, y = threadIdx.x >> 4;
  tile[y][x] = dz[((size_t)h * NM + tj + y) * NM + ti + x];            // dz[j][i]
  __syncthreads();
  const int col = tj + x;
  const size_t o = ((size_t)h * NM + ti + y) * NM + col;
  da2[o] += tile[x][y] / den + (csum[(size_t)h * NM + col] == mc ? share : 0.f);
}
// ds = a (da - rowsum(da . a)), in place over da: block (row, head)
__global__ __launch_bounds__(256) void nysb_softmax_bwd_kernel(const float* __restrict__ a2, float* __restrict__ da2) {
  __shared__ float red[256];
  const int t = threadIdx.x;
  const size_t o = ((size_t)blockIdx.y * NM + blockIdx.x) * NM + t;
  const float a = a2[o], d = da2[o];
  red[t] = a * d;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  da2[o] = a * (d - red[0]);
}
// a -= b
__global__ __launch_bounds__(256) void nysb_sub_kernel(float* __restrict__ a, const float* __restrict__ b, size_t n4) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  float4 x = ((float4*)a)[i];
  const float4 y = ((const float4*)b)[i];
  x.x -= y.x;
  x.y -= y.y;
  x.z -= y.z;
  x.w -= y.w;
  ((float4*)a)[i] = x;
}

// ---- landmarks backward: block (row t, q | k, item): d_qkv[t, third, c] += d[h, t / l, c % 64] / l
__global__ void nysb_landmarks_kernel(const float* __restrict__ d_ql, const float* __restrict__ d_kl, float* __restrict__ d_qkv,
                                      int l, int heads) {
  const int hd = heads * ND, c = threadIdx.x;
  if (c >= hd) return;
  const size_t t = blockIdx.x, item = blockIdx.z;
  const float* src = blockIdx.y ? d_kl : d_ql;
  d_qkv[(item * gridDim.x + t) * 3 * hd + (size_t)blockIdx.y * hd + c] +=
      src[((item * heads + (size_t)(c >> 6)) * NM + t / l) * ND + (c & 63)] / (float)l;
}

// the q columns of rows [0, rows) times 64^-0.5 (the forward scales q in the qkv linear's epilogue)
__global__ __launch_bounds__(256) void nysb_scale_q_kernel(float* __restrict__ d_qkv, size_t rows, int hd) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * hd) return;
  const size_t r = i / hd, c = i - r * hd;
  d_qkv[r * 3 * hd + c] *= 0.125f;
}

}  // namespace

// chunk partials of the output backward: dW | dkl [b, heads, nch, 256, 64] each, dconv_w [b, heads, nch, 64]
size_t nystrom_output_bwd_floats(long np, int heads, int b) {
  int nsub, spc, nch;
  nystrom_chunks(np, &nsub, &spc, &nch);
  return (size_t)b * heads * nch * (2 * NM * ND + 64);
}
// of the landmark-attention backward: dql [b, heads, nch, 256, 64] | d3 [b, heads, 256]
size_t nystrom_lattn_bwd_floats(long np, int heads, int b) {
  int nsub, spc, nch;
  nystrom_chunks(np, &nsub, &spc, &nch);
  return (size_t)b * heads * nch * NM * ND + (size_t)b * heads * NM;
}
// per matrix (b * heads of them): z_0 .. z_{iters-1} | xz, t1, t2, t3, dta, dtb, dxz, dz, dz', da2 | row sums, column sums;
// then 64 scalars | one partial per matrix, in whole runs of 64 (b = 1: the 64 + 64 of the single-sequence carve)
size_t nystrom_pinv_bwd_floats(int heads, int iters, int b) {
  const size_t nmat = (size_t)b * heads;
  return nmat * NM * NM * (iters + 10) + nmat * NM * 2 + 64 + (nmat + 63) / 64 * 64;
}

hipError_t launch_nystrom_output_backward(const float* qkv, const float* kl, const float* wz, const float* conv_w,
                                          const float* d_o, float* d_qkv, float* d_kl, float* d_wz, float* d_conv_w, float* ws,
                                          long np, int heads, int ks, hipStream_t st, int b) {
  int nsub, spc, nch;
  nystrom_chunks(np, &nsub, &spc, &nch);
  const int hb = b * heads;
  float* pW = ws;
  float* pK = pW + (size_t)hb * nch * NM * ND;
  float* pC = pK + (size_t)hb * nch * NM * ND;
  nysb_output_kernel<<<dim3(nch, heads, b), 256, 0, st>>>(qkv, kl, wz, conv_w, d_o, d_qkv, pW, pK, pC, (int)np, heads, ks, nsub, spc);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  nysb_merge_kernel<<<dim3(NM * ND / 256, hb), 256, 0, st>>>(pW, d_wz, nch, NM * ND, NM * ND, 0, 1);
  nysb_merge_kernel<<<dim3(NM * ND / 256, hb), 256, 0, st>>>(pK, d_kl, nch, NM * ND, NM * ND, 0, 1);
  if (conv_w) nysb_merge_kernel<<<dim3(1, heads), 256, 0, st>>>(pC, d_conv_w, nch, 64, ks, 0, b);   // summed over the items
  return hipGetLastError();
}

hipError_t launch_nystrom_zav_backward(const float* z, const float* av, const float* d_wz, float* d_z, float* d_av, int heads,
                                       hipStream_t st, int b) {
  hipError_t e = gemm(false, true, d_wz, av, d_z, nullptr, NM, NM, ND, b * heads, 1.f, 0.f, 0.f, 0.f, 0, st);   // dW AV^T
  if (e != hipSuccess) return e;
  return gemm(true, false, z, d_wz, d_av, nullptr, NM, ND, NM, b * heads, 1.f, 0.f, 0.f, 0.f, 0, st);          // Z^T dW
}

hipError_t launch_nystrom_lattn_backward(const float* qkv, const float* ql, const float* av, const float* lse, const float* d_av,
                                         float* d_qkv, float* d_ql, float* ws, long np, int heads, hipStream_t st, int b) {
  int nsub, spc, nch;
  nystrom_chunks(np, &nsub, &spc, &nch);
  const int hb = b * heads;
  float* pQ = ws;
  float* d3 = pQ + (size_t)hb * nch * NM * ND;
  nysb_rowdot_kernel<<<dim3(hb * NM / 4), 256, 0, st>>>(d_av, av, d3, hb * NM);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  nysb_lattn_kernel<<<dim3(nch, heads, b), 256, 0, st>>>(qkv, ql, lse, d3, d_av, d_qkv, pQ, heads, nsub, spc);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  nysb_merge_kernel<<<dim3(NM * ND / 256, hb), 256, 0, st>>>(pQ, d_ql, nch, NM * ND, NM * ND, 0, 1);
  return hipGetLastError();
}

// d_ql, d_kl (+)= the gradient of pinv_iter(a2 = softmax(ql kl^T), iters) under d_z.  b items: every matrix of every item is
// a "head" below -- den, its ties and d den are taken over all of them
hipError_t launch_nystrom_pinv_sim_backward(const float* ql, const float* kl, const float* a2, const float* d_z, float* d_ql,
                                            float* d_kl, int accumulate, float* ws, int heads_per_item, int iters, hipStream_t st,
                                            int b) {
  const int heads = b * heads_per_item;
  const size_t all = (size_t)NM * NM * heads;
  float* zs = ws;
  float* xz = zs + all * iters;
  float* t1 = xz + all;
  float* t2 = t1 + all;
  float* t3 = t2 + all;
  float* dta = t3 + all;
  float* dtb = dta + all;
  float* dxz = dtb + all;
  float* dz = dxz + all;
  float* dzn = dz + all;
  float* da2 = dzn + all;
  float* rsum = da2 + all;
  float* csum = rsum + (size_t)heads * NM;
  float* scal = csum + (size_t)heads * NM;
  float* part = scal + 64;
  hipError_t e;
#define NYSB_TRY(call)               \
  do {                               \
    e = (call);                      \
    if (e != hipSuccess) return e;   \
  } while (0)
  nysb_sums_kernel<<<heads, 256, 0, st>>>(a2, rsum, csum);
  nysb_scal_kernel<<<1, 256, 0, st>>>(rsum, csum, scal, heads * NM);
  nysb_z0_kernel<<<dim3(NM / 16, NM / 16, heads), 256, 0, st>>>(a2, scal, zs);
  NYSB_TRY(hipGetLastError());
  // xz = a2 z ; t1 = 7 I - xz ; t2 = 15 I - xz t1 ; t3 = 13 I - xz t2
  auto terms = [&](const float* z) -> hipError_t {
    hipError_t r = gemm(false, false, a2, z, xz, t1, NM, NM, NM, heads, 1.f, 0.f, -1.f, 7.f, 0, st);
    if (r == hipSuccess) r = gemm(false, false, xz, t1, t2, nullptr, NM, NM, NM, heads, -1.f, 15.f, 0.f, 0.f, 0, st);
    if (r == hipSuccess) r = gemm(false, false, xz, t2, t3, nullptr, NM, NM, NM, heads, -1.f, 13.f, 0.f, 0.f, 0, st);
    return r;
  };
  // The forward sweep keeps every iterate and carries the tangent zd = d z_i / d log(scale of z0) along (zd_0 = z0):
  // sum(d_z . zd_iters) is the derivative through den.  Read off the reverse sweep as sum(dz_0 . z_0) it is a sum of terms
  // ~1e5 times its own size whenever the iteration has converged (z no longer depends on its start): fp32 noise there
  // outweighs the whole gradient behind the softmax backward.  The tangent shrinks with the convergence instead.
  float *zd = dta, *zdn = dtb, *xzd = dxz, *t2d = dzn, *t3d = da2;     // (the reverse sweep's buffers, not yet in use)
  NYSB_TRY(hipMemcpyAsync(zd, zs, all * sizeof(float), hipMemcpyDeviceToDevice, st));
  for (int i = 0; i < iters; ++i) {
    const float* z = zs + all * i;
    NYSB_TRY(terms(z));
    NYSB_TRY(gemm(false, false, a2, zd, xzd, nullptr, NM, NM, NM, heads, 1.f, 0.f, 0.f, 0.f, 0, st));       // xz' = a2 z'
    NYSB_TRY(gemm(false, false, xz, xzd, t2d, nullptr, NM, NM, NM, heads, 1.f, 0.f, 0.f, 0.f, 0, st));      // t2' = xz xz' - xz' t1
    NYSB_TRY(gemm(false, false, xzd, t1, t2d, nullptr, NM, NM, NM, heads, -1.f, 0.f, 0.f, 0.f, 1, st));
    NYSB_TRY(gemm(false, false, xzd, t2, t3d, nullptr, NM, NM, NM, heads, -1.f, 0.f, 0.f, 0.f, 0, st));     // t3' = -xz' t2 - xz t2'
    NYSB_TRY(gemm(false, false, xz, t2d, t3d, nullptr, NM, NM, NM, heads, -1.f, 0.f, 0.f, 0.f, 1, st));
    NYSB_TRY(gemm(false, false, zd, t3, zdn, nullptr, NM, NM, NM, heads, 0.25f, 0.f, 0.f, 0.f, 0, st));     // z'' = 1/4 (z' t3 + z t3')
    NYSB_TRY(gemm(false, false, z, t3d, zdn, nullptr, NM, NM, NM, heads, 0.25f, 0.f, 0.f, 0.f, 1, st));
    float* sw = zd;
    zd = zdn;
    zdn = sw;
    if (i + 1 < iters)
      NYSB_TRY(gemm(false, false, z, t3, zs + all * (i + 1), nullptr, NM, NM, NM, heads, 0.25f, 0.f, 0.f, 0.f, 0, st));
  }
  nysb_dot_kernel<<<heads, 256, 0, st>>>(d_z, zd, part);
  nysb_tot_kernel<<<1, 256, 0, st>>>(part, scal, heads);
  NYSB_TRY(hipGetLastError());
  NYSB_TRY(hipMemcpyAsync(dz, d_z, all * sizeof(float), hipMemcpyDeviceToDevice, st));
  for (int i = iters - 1; i >= 0; --i) {
    const float* z = zs + all * i;
    if (i != iters - 1) NYSB_TRY(terms(z));                  // (xz .. t3 of the last iterate are still there)
    NYSB_TRY(gemm(true, false, z, dz, dta, nullptr, NM, NM, NM, heads, 0.25f, 0.f, 0.f, 0.f, 0, st));      // dt3 = 1/4 z^T dz
    NYSB_TRY(gemm(false, true, dz, t3, dzn, nullptr, NM, NM, NM, heads, 0.25f, 0.f, 0.f, 0.f, 0, st));     // dz_i = 1/4 dz t3^T
    NYSB_TRY(gemm(false, true, dta, t2, dxz, nullptr, NM, NM, NM, heads, -1.f, 0.f, 0.f, 0.f, 0, st));     // dxz = -dt3 t2^T
    NYSB_TRY(gemm(true, false, xz, dta, dtb, nullptr, NM, NM, NM, heads, -1.f, 0.f, 0.f, 0.f, 0, st));     // dt2 = -xz^T dt3
    NYSB_TRY(gemm(false, true, dtb, t1, dxz, nullptr, NM, NM, NM, heads, -1.f, 0.f, 0.f, 0.f, 1, st));     // dxz -= dt2 t1^T
    NYSB_TRY(gemm(true, false, xz, dtb, dta, nullptr, NM, NM, NM, heads, -1.f, 0.f, 0.f, 0.f, 0, st));     // dt1 = -xz^T dt2
    nysb_sub_kernel<<<dim3((unsigned)(all / 4 / 256)), 256, 0, st>>>(dxz, dta, all / 4);                   // dxz -= dt1
    NYSB_TRY(hipGetLastError());
    NYSB_TRY(gemm(false, true, dxz, z, da2, nullptr, NM, NM, NM, heads, 1.f, 0.f, 0.f, 0.f, i != iters - 1, st));  // da2 += dxz z^T
    NYSB_TRY(gemm(true, false, a2, dxz, dzn, nullptr, NM, NM, NM, heads, 1.f, 0.f, 0.f, 0.f, 1, st));      // dz = dz_i + a2^T dxz
    float* sw = dz;
    dz = dzn;
    dzn = sw;
  }
  // z0 = a2^T / den
  nysb_da2_z0_kernel<<<dim3(NM / 16, NM / 16, heads), 256, 0, st>>>(da2, dz, csum, scal);
  nysb_softmax_bwd_kernel<<<dim3(NM, heads), 256, 0, st>>>(a2, da2);
  NYSB_TRY(hipGetLastError());
  NYSB_TRY(gemm(false, false, da2, kl, d_ql, nullptr, NM, ND, NM, heads, 1.f, 0.f, 0.f, 0.f, accumulate, st));   // dS2 kl
  NYSB_TRY(gemm(true, false, da2, ql, d_kl, nullptr, NM, ND, NM, heads, 1.f, 0.f, 0.f, 0.f, accumulate, st));    // dS2^T ql
#undef NYSB_TRY
  return hipSuccess;
}

hipError_t launch_nystrom_landmarks_backward(const float* d_ql, const float* d_kl, float* d_qkv, long np, int heads,
                                             hipStream_t st, int b) {
  nysb_landmarks_kernel<<<dim3((unsigned)np, 2, b), heads * ND, 0, st>>>(d_ql, d_kl, d_qkv, (int)(np / NM), heads);
  return hipGetLastError();
}

hipError_t launch_nystrom_scale_q(float* d_qkv, long rows, int heads, hipStream_t st) {
  const size_t n = (size_t)rows * heads * ND;
  nysb_scale_q_kernel<<<dim3((unsigned)((n + 255) / 256)), 256, 0, st>>>(d_qkv, (size_t)rows, heads * ND);
  return hipGetLastError();
}
