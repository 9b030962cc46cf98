// nystrom.hip -- Nystrom attention (modules/nystrom_attention.py:67-149), the hot path of the TransMIL baseline
// (modules/transmil.py), inference.  Exact fp32; every matrix product runs on v_mfma_f32_16x16x4_f32.  No atomics, every sum
// has a fixed order: the same inputs give the same bits.
//
// Layout.  qkv [np, 3 * heads * 64] as the qkv linear wrote it (q columns scaled), np = 256 * l rows, the first np - n of them
// zero (the FRONT padding of the reference).  Head hh owns columns hh * 64 .. of each of the q | k | v thirds.
//   landmarks   ql, kl [heads, 256, 64] : means of l consecutive rows
//   sim2        a2 [heads, 256, 256]    = softmax(ql kl^T)
//   scale       one scalar over ALL heads: max row abs sum * max column abs sum of a2 ; z0 = a2^T / scale
//   bmm         the pinv iteration's GEMMs, C = s (A B) + t I (optionally a second output from the same accumulators)
//   lattn       av [heads, 256, 64] = softmax(ql k^T) v : keys split into chunks, one (max, sum, acc) record per chunk and
//               landmark, merged in chunk order
//   output      o [np, heads * 64] = softmax(q kl^T) w + conv(v),  w = z av
// Batch.  Every kernel takes b sequences in one launch: qkv [b, np, 3 * heads * 64] and o [b, np, heads * 64] item by item (each
// with its own front padding; the stencil stays inside its item), everything else [b, heads, ...] -- matrix b * heads + h.  The
// item is the grid's last dimension, so that b = 1 is the single-sequence launch, block for block.  The scale is ONE scalar over
// all b * heads matrices (the reference's torch.max over the whole batch).
// Every block is 256 threads = 4 waves; a wave owns 16 rows x 64 columns of the block's 64 x 64 tile (four 16 x 16 MFMA
// accumulators; the batched GEMM uses 64 x 32 tiles, two accumulators).  Operand tiles go through LDS: A as [row][k] with a row stride of 4 (mod 32) floats, B as [k][column] with a
// row stride of 16 (mod 64) floats, so that the 64 lanes of one operand read hit 64 different banks.
#include "nystrom_tiles.h"

namespace {

// ---- landmarks: block (landmark j, q | k, item), thread = one of the heads * 64 columns
__global__ void nys_landmarks_kernel(const float* __restrict__ qkv, float* __restrict__ ql, float* __restrict__ kl, int l,
                                     int heads) {
  const int hd = heads * ND, c = threadIdx.x, j = blockIdx.x;
  if (c >= hd) return;
  const size_t ld3 = (size_t)3 * hd;
  const float* src = qkv + ((size_t)blockIdx.z * NM + j) * l * ld3 + (size_t)blockIdx.y * hd + c;
  float s = 0.f;
  for (int i = 0; i < l; ++i) s += src[(size_t)i * ld3];
  float* dst = blockIdx.y ? kl : ql;
  dst[(((size_t)blockIdx.z * heads + (c >> 6)) * NM + j) * ND + (c & 63)] = s / (float)l;
}

// ---- a2 = softmax(ql kl^T): block (64-row tile, head, item)
__global__ __launch_bounds__(256) void nys_sim2_kernel(const float* __restrict__ ql, const float* __restrict__ kl,
                                                       float* __restrict__ a2) {
  __shared__ __attribute__((aligned(16))) float As[64 * LDA];
  __shared__ __attribute__((aligned(16))) float Bs[64 * LDB];
  const int h = blockIdx.z * gridDim.y + blockIdx.y, r0 = blockIdx.x * 64, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  stage_rows(As, LDA, ql + ((size_t)h * NM + r0) * ND, ND, 64);
  f32x4 s[4][4];
  scores_softmax_256(As, Bs, kl + (size_t)h * NM * ND, s);
  float* out = a2 + ((size_t)h * NM + r0 + 16 * w + 4 * (lane >> 4)) * NM + (lane & 15);
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int j = 0; j < 4; ++j) out[(size_t)r * NM + 64 * ct + 16 * j] = s[ct][j][r];
}

// ---- the pinv's initial scale: per matrix (head, item) the largest row abs sum and the largest column abs sum -> sp[2 h],
// sp[2 h + 1]
__global__ __launch_bounds__(256) void nys_scale_part_kernel(const float* __restrict__ a2, float* __restrict__ sp) {
  __shared__ float red[2][256];
  const int h = blockIdx.y * gridDim.x + blockIdx.x, t = threadIdx.x;
  const float* a = a2 + (size_t)h * NM * NM;
  float rs = 0.f, cs = 0.f;
  for (int i = 0; i < NM; ++i) {
    rs += fabsf(a[(size_t)t * NM + i]);
    cs += fabsf(a[(size_t)i * NM + t]);
  }
  red[0][t] = rs;
  red[1][t] = cs;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
      red[0][t] = fmaxf(red[0][t], red[0][t + o]);
      red[1][t] = fmaxf(red[1][t], red[1][t + o]);
    }
    __syncthreads();
  }
  if (t == 0) {
    sp[2 * h] = red[0][0];
    sp[2 * h + 1] = red[1][0];
  }
}

// more than NYS_SCALE_LOOP matrices: their records folded into one (sp[2 n], sp[2 n + 1]) by one block -- a strided pass per
// thread, then the tree.  (max is exact and order-free, and the order is fixed anyway.)
constexpr int NYS_SCALE_LOOP = 16;
__global__ __launch_bounds__(256) void nys_scale_reduce_kernel(float* __restrict__ sp, int n) {
  __shared__ float red[2][256];
  const int t = threadIdx.x;
  float mr = 0.f, mc = 0.f;                  // (abs sums: 0 is the identity)
  for (int i = t; i < n; i += 256) {
    mr = fmaxf(mr, sp[2 * i]);
    mc = fmaxf(mc, sp[2 * i + 1]);
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
  if (t == 0) {
    sp[2 * n] = red[0][0];
    sp[2 * n + 1] = red[1][0];
  }
}

// z0 = a2^T / (max over ALL matrices of the row sums * max over all of them of the column sums; sp holds `nparts` records):
// block (16 x 16 tile pair, head, item)
__global__ __launch_bounds__(256) void nys_z0_kernel(const float* __restrict__ a2, const float* __restrict__ sp,
                                                     float* __restrict__ z, int nparts) {
  __shared__ float tile[16][17];
  float mr = sp[0], mc = sp[1];
  for (int i = 1; i < nparts; ++i) {
    mr = fmaxf(mr, sp[2 * i]);
    mc = fmaxf(mc, sp[2 * i + 1]);
  }
  const float denom = mr * mc;
  const int h = blockIdx.z * gridDim.y + blockIdx.y, ti = (blockIdx.x >> 4) * 16, tj = (blockIdx.x & 15) * 16;
  const int x = threadIdx.x & 15, y = threadIdx.x >> 4;
  tile[y][x] = a2[((size_t)h * NM + tj + y) * NM + ti + x];          // a2[j][i]
  __syncthreads();
  z[((size_t)h * NM + ti + y) * NM + tj + x] = tile[x][y] / denom;    // z[i][j] = a2[j][i] / denom
}

// ---- batched GEMM with the iteration's epilogue: C = s (A B) + t I, and optionally C2 = s2 (A B) + t2 I.
// A [M, K], B [K, N], row-major with leading dimensions; M a multiple of 64, N and K of 32.  block ((M / 64, N / 32), head, item):
// (N / 32 a power of two) a 64 x 32 tile, so that the 256 x 256 products of 8 heads are 256 blocks (one per CU); the next k-step's tiles are loaded
// into registers while the matrix cores work on the current one.
struct BmmArgs {
  const float *A, *B;
  float *C, *C2;
  int K, lda, ldb, ldc, lx;      // 2^lx = N / 32 tiles per tile row
  size_t sA, sB, sC;
  float s, t, s2, t2;
};
constexpr int BK = 32, BN = 32, LDA32 = 36, LDB32 = 48;
__global__ __launch_bounds__(256) void nys_bmm_kernel(const BmmArgs p) {
  __shared__ __attribute__((aligned(16))) float As[64 * LDA32];
  __shared__ __attribute__((aligned(16))) float Bs[BK * LDB32];
  const int b = blockIdx.z * gridDim.y + blockIdx.y, m0 = (blockIdx.x >> p.lx) * 64, n0 = (blockIdx.x & ((1 << p.lx) - 1)) * BN, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float* A = p.A + b * p.sA + (size_t)m0 * p.lda;
  const float* B = p.B + b * p.sB + n0;
  const int ar = tid >> 3, ac = (tid & 7) * 4;          // A tile 64 x 32: rows ar and ar + 32; B tile 32 x 32: row ar
  float4 ra0, ra1, rb;
  auto load = [&](int k0) {
    ra0 = *(const float4*)(A + (size_t)ar * p.lda + k0 + ac);
    ra1 = *(const float4*)(A + (size_t)(ar + 32) * p.lda + k0 + ac);
    rb = *(const float4*)(B + (size_t)(k0 + ar) * p.ldb + ac);
  };
  f32x4 acc[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  load(0);
  for (int k0 = 0; k0 < p.K; k0 += BK) {
    __syncthreads();
    *(float4*)(As + ar * LDA32 + ac) = ra0;
    *(float4*)(As + (ar + 32) * LDA32 + ac) = ra1;
    *(float4*)(Bs + ar * LDB32 + ac) = rb;
    __syncthreads();
    if (k0 + BK < p.K) load(k0 + BK);
    mma_16x64<2>(As + w * 16 * LDA32, LDA32, Bs, LDB32, BK, acc);
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
      p.C[o] = p.s * acc[j][r] + p.t * d;
      if (p.C2) p.C2[o] = p.s2 * acc[j][r] + p.t2 * d;
    }
  }
}

// ---- landmark attention over the keys, one chunk: block (chunk, (64-landmark tile, head), item).  The chunk's keys go by in
// sub-chunks of 64 with an online softmax; the block leaves pm / ps [heads, nch, 256] and pacc [heads, nch, 256, 64].
__global__ __launch_bounds__(256) void nys_lattn_part_kernel(const float* __restrict__ qkv, const float* __restrict__ ql,
                                                             float* __restrict__ pm, float* __restrict__ ps,
                                                             float* __restrict__ pacc, int nsub, int sub_per_chunk, int heads) {
  __shared__ __attribute__((aligned(16))) float Qs[64 * LDA];
  __shared__ __attribute__((aligned(16))) float Kt[64 * LDB];          // k^T of the sub-chunk, then its probabilities
  __shared__ __attribute__((aligned(16))) float Vs[64 * LDB];
  float* Ps = Kt;                                                        // [64][LDA]
  const int ch = blockIdx.x, r0 = (blockIdx.y & 3) * 64, h = blockIdx.y >> 2, nch = gridDim.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, hd = heads * ND;
  const size_t ld3 = (size_t)3 * hd, bh = (size_t)blockIdx.z * heads + h;
  qkv += (size_t)blockIdx.z * nsub * 64 * ld3;
  stage_rows(Qs, LDA, ql + (bh * NM + r0) * ND, ND, 64);
  const int s_begin = ch * sub_per_chunk, s_end = min(nsub, s_begin + sub_per_chunk);
  float m[4], sum[4];
  f32x4 o[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m[r] = -INFINITY;
    sum[r] = 0.f;
    o[r] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int sc = s_begin; sc < s_end; ++sc) {
    const float* krow = qkv + (size_t)sc * 64 * ld3 + hd + (size_t)h * ND;
    __syncthreads();                       // the previous sub-chunk's reads of Ps / Vs are done
    stage_64x64_t(Kt, LDB, krow, ld3);
    stage_rows(Vs, LDB, krow + hd, ld3, 64);
    __syncthreads();
    f32x4 s[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    mma_16x64(Qs + w * 16 * LDA, LDA, Kt, LDB, ND, s);
    __syncthreads();                       // every wave has read Kt: it becomes Ps
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float mx = fmaxf(fmaxf(s[0][r], s[1][r]), fmaxf(s[2][r], s[3][r]));
      mx = fmaxf(m[r], row16_max(mx));
      const float scale = expf(m[r] - mx);  // 0 on the first sub-chunk (m = -inf)
      m[r] = mx;
      float psum = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float p = expf(s[j][r] - mx);
        psum += p;
        Ps[(16 * w + 4 * (lane >> 4) + r) * LDA + 16 * j + (lane & 15)] = p;
      }
      sum[r] = sum[r] * scale + row16_sum(psum);
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j][r] *= scale;
    }
    __syncthreads();
    mma_16x64(Ps + w * 16 * LDA, LDA, Vs, LDB, 64, o);
  }
  const size_t rec = (bh * nch + ch) * NM + r0 + 16 * w + 4 * (lane >> 4);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if ((lane & 15) == 0) {
      pm[rec + r] = m[r];
      ps[rec + r] = sum[r];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) pacc[(rec + r) * ND + 16 * j + (lane & 15)] = o[j][r];
  }
}

// merge of the chunk records in chunk order: block (4 landmarks, head, item), thread = (landmark, column)
__global__ __launch_bounds__(256) void nys_lattn_merge_kernel(const float* __restrict__ pm, const float* __restrict__ ps,
                                                              const float* __restrict__ pacc, float* __restrict__ av, int nch,
                                                              float* __restrict__ lse) {
  const int h = blockIdx.z * gridDim.y + blockIdx.y, row = blockIdx.x * 4 + (threadIdx.x >> 6), d = threadIdx.x & 63;
  const size_t base = (size_t)h * nch * NM + row;
  float M = -INFINITY;
  for (int c = 0; c < nch; ++c) M = fmaxf(M, pm[base + (size_t)c * NM]);
  float sum = 0.f, acc = 0.f;
  for (int c = 0; c < nch; ++c) {
    const float e = expf(pm[base + (size_t)c * NM] - M);
    sum += ps[base + (size_t)c * NM] * e;
    acc += pacc[(base + (size_t)c * NM) * ND + d] * e;
  }
  av[((size_t)h * NM + row) * ND + d] = acc / sum;
  if (lse && d == 0) lse[(size_t)h * NM + row] = M + logf(sum);     // (the backward's row log-sum-exp; av is untouched by it)
}

// ---- output: block (64-token tile, head, item): softmax(q kl^T) w + the depth-wise stencil over v, written head-merged
constexpr int OUT_LDS_FLOATS = 64 * LDA + 64 * LDB + 64 * LDA;          // Qs | Bs | Ps ; the v tile reuses all of it
__global__ __launch_bounds__(256) void nys_output_kernel(const float* __restrict__ qkv, const float* __restrict__ kl,
                                                         const float* __restrict__ wz, const float* __restrict__ conv_w,
                                                         float* __restrict__ out, int np, int heads, int ks) {
  __shared__ __attribute__((aligned(16))) float lds[OUT_LDS_FLOATS];
  float* Qs = lds;
  float* Bs = lds + 64 * LDA;
  float* Ps = Bs + 64 * LDB;
  const int t0 = blockIdx.x * 64, h = blockIdx.y, hd = heads * ND;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const size_t ld3 = (size_t)3 * hd, bh = (size_t)blockIdx.z * heads + h;
  qkv += (size_t)blockIdx.z * np * ld3;
  out += (size_t)blockIdx.z * np * hd;
  stage_rows(Qs, LDA, qkv + (size_t)t0 * ld3 + (size_t)h * ND, ld3, 64);
  f32x4 s[4][4];
  scores_softmax_256(Qs, Bs, kl + bh * NM * ND, s);
  f32x4 o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int j = 0; j < 4; ++j) Ps[(16 * w + 4 * (lane >> 4) + r) * LDA + 16 * j + (lane & 15)] = s[ct][j][r];
    stage_rows(Bs, LDB, wz + (bh * NM + ct * 64) * ND, ND, 64);
    __syncthreads();
    mma_16x64(Ps + w * 16 * LDA, LDA, Bs, LDB, 64, o);
  }
  if (conv_w) {
    // v rows t0 - half .. t0 + 63 + half of this head (zero outside the padded sequence): (64 + 2 half) x 64 <= 8064 floats
    const int half = ks >> 1, rows = 64 + 2 * half;
    float* Vs = lds;
    __syncthreads();
    for (int i = threadIdx.x; i < rows * 16; i += 256) {
      const int r = i >> 4, c = (i & 15) * 4, t = t0 - half + r;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (t >= 0 && t < np) v = *(const float4*)(qkv + (size_t)t * ld3 + 2 * hd + (size_t)h * ND + c);
      *(float4*)(Vs + r * 64 + c) = v;
    }
    __syncthreads();
    const float* cw = conv_w + (size_t)h * ks;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * w + 4 * (lane >> 4) + r;
      float c4[4] = {0.f, 0.f, 0.f, 0.f};
      for (int tap = 0; tap < ks; ++tap) {
        const float wt = cw[tap];
        const float* vp = Vs + (row + tap) * 64 + (lane & 15);
#pragma unroll
        for (int j = 0; j < 4; ++j) c4[j] += wt * vp[16 * j];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j][r] += c4[j];
    }
  }
  float* dst = out + (size_t)(t0 + 16 * w + 4 * (lane >> 4)) * hd + (size_t)h * ND + (lane & 15);
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int j = 0; j < 4; ++j) dst[(size_t)r * hd + 16 * j] = o[j][r];
}

// TransMIL's sequence: row 0 = cls, rows 1 .. N = h, rows N + 1 .. H*H = the first H*H - N rows of h again (a wrap)
__global__ __launch_bounds__(256) void transmil_assemble_kernel(const float* __restrict__ h, const float* __restrict__ cls,
                                                                float* __restrict__ seq, int N, int rows, int dim4) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)rows * dim4) return;
  const size_t r = i / dim4, c = i - r * dim4;
  const float4* src = r == 0 ? (const float4*)cls + c : (const float4*)h + (r - 1 < (size_t)N ? r - 1 : r - 1 - N) * dim4 + c;
  ((float4*)seq)[i] = *src;
}

// logits[c] = w[c] . x + b[c] for one row x [dim] (TransMIL's _fc2 on the cls row): one block, a wave per class in turn
__global__ __launch_bounds__(256) void transmil_head_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ b, float* __restrict__ logits, int dim,
                                                            int n_classes) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int c = wv; c < n_classes; c += 4) {
    float s = 0.f;
    for (int i = lane; i < dim; i += 64) s += x[i] * w[(size_t)c * dim + i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) logits[c] = s + (b ? b[c] : 0.f);
  }
}

hipError_t bmm(const float* A, const float* B, float* C, float* C2, int M, int N, int K, int heads, int b, size_t sA, size_t sB,
               size_t sC, float s, float t, float s2, float t2, hipStream_t st) {
  BmmArgs p{A, B, C, C2, K, K, N, N, __builtin_ctz((unsigned)(N / BN)), sA, sB, sC, s, t, s2, t2};
  nys_bmm_kernel<<<dim3((N / BN) * (M / 64), heads, b), 256, 0, st>>>(p);
  return hipGetLastError();
}

}  // namespace

// chunks of the landmark attention: at most NYS_MAX_CHUNKS records per (head, landmark), whole sub-chunks of 64 keys
constexpr int NYS_MAX_CHUNKS = 32;
void nystrom_chunks(long np, int* nsub, int* sub_per_chunk, int* nch) {
  *nsub = (int)(np / 64);
  *sub_per_chunk = (*nsub + NYS_MAX_CHUNKS - 1) / NYS_MAX_CHUNKS;
  *nch = (*nsub + *sub_per_chunk - 1) / *sub_per_chunk;
}
size_t nystrom_lattn_floats(long np, int heads, int b) {
  int nsub, spc, nch;
  nystrom_chunks(np, &nsub, &spc, &nch);
  return (size_t)b * heads * nch * NM * (ND + 2);
}
// z', xz, t1, t2 | the scale records: one per matrix and, beyond NYS_SCALE_LOOP of them, their fold
size_t nystrom_pinv_floats(int heads, int b) {
  const size_t nmat = (size_t)b * heads;
  return nmat * NM * NM * 4 + 64 + (nmat > NYS_SCALE_LOOP ? 2 * nmat : 0);
}

hipError_t launch_nystrom_landmarks(const float* qkv, float* ql, float* kl, long np, int heads, hipStream_t st, int b) {
  nys_landmarks_kernel<<<dim3(NM, 2, b), heads * ND, 0, st>>>(qkv, ql, kl, (int)(np / NM), heads);
  return hipGetLastError();
}

hipError_t launch_nystrom_sim2(const float* ql, const float* kl, float* a2, int heads, hipStream_t st, int b) {
  nys_sim2_kernel<<<dim3(NM / 64, heads, b), 256, 0, st>>>(ql, kl, a2);
  return hipGetLastError();
}

hipError_t launch_nystrom_lattn(const float* qkv, const float* ql, float* av, float* ws, long np, int heads, hipStream_t st,
                                float* lse, int b) {
  int nsub, spc, nch;
  nystrom_chunks(np, &nsub, &spc, &nch);
  const size_t recs = (size_t)b * heads * nch * NM;
  float* pm = ws;
  float* ps = pm + recs;
  float* pacc = ps + recs;
  nys_lattn_part_kernel<<<dim3(nch, (NM / 64) * heads, b), 256, 0, st>>>(qkv, ql, pm, ps, pacc, nsub, spc, heads);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  nys_lattn_merge_kernel<<<dim3(NM / 4, heads, b), 256, 0, st>>>(pm, ps, pacc, av, nch, lse);
  return hipGetLastError();
}

// z [b, heads, 256, 256] = the iterated pseudo-inverse of a2; ws: nystrom_pinv_floats(heads, b) floats
hipError_t launch_nystrom_pinv(const float* a2, float* z, float* ws, int heads, int iters, hipStream_t st, int b) {
  const int nmat = b * heads;
  const size_t mat = (size_t)NM * NM, all = mat * nmat;
  float* zb = ws;
  float* xz = zb + all;
  float* t1 = xz + all;
  float* t2 = t1 + all;
  float* sp = t2 + all;
  // the last iteration must land in z: start in whichever buffer makes that so
  float* cur = (iters % 2) ? zb : z;
  float* nxt = (iters % 2) ? z : zb;
  nys_scale_part_kernel<<<dim3(heads, b), 256, 0, st>>>(a2, sp);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const bool fold = nmat > NYS_SCALE_LOOP;
  if (fold) {
    nys_scale_reduce_kernel<<<1, 256, 0, st>>>(sp, nmat);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  nys_z0_kernel<<<dim3((NM / 16) * (NM / 16), heads, b), 256, 0, st>>>(a2, fold ? sp + 2 * (size_t)nmat : sp, cur, fold ? 1 : nmat);
  e = hipGetLastError();
  for (int it = 0; it < iters && e == hipSuccess; ++it) {
    // xz = a2 z ; t1 = 7 I - xz ; t2 = 15 I - xz t1 ; t1 = 13 I - xz t2 ; z' = 1/4 z t1
    e = bmm(a2, cur, xz, t1, NM, NM, NM, heads, b, mat, mat, mat, 1.f, 0.f, -1.f, 7.f, st);
    if (e == hipSuccess) e = bmm(xz, t1, t2, nullptr, NM, NM, NM, heads, b, mat, mat, mat, -1.f, 15.f, 0.f, 0.f, st);
    if (e == hipSuccess) e = bmm(xz, t2, t1, nullptr, NM, NM, NM, heads, b, mat, mat, mat, -1.f, 13.f, 0.f, 0.f, st);
    if (e == hipSuccess) e = bmm(cur, t1, nxt, nullptr, NM, NM, NM, heads, b, mat, mat, mat, 0.25f, 0.f, 0.f, 0.f, st);
    float* sw = cur;
    cur = nxt;
    nxt = sw;
  }
  return e;
}

hipError_t launch_nystrom_zav(const float* z, const float* av, float* wz, int heads, hipStream_t st, int b) {
  return bmm(z, av, wz, nullptr, NM, ND, NM, heads, b, (size_t)NM * NM, (size_t)NM * ND, (size_t)NM * ND, 1.f, 0.f, 0.f, 0.f, st);
}

hipError_t launch_nystrom_output(const float* qkv, const float* kl, const float* wz, const float* conv_w, float* o, long np,
                                 int heads, int ks, hipStream_t st, int b) {
  nys_output_kernel<<<dim3((unsigned)(np / 64), heads, b), 256, 0, st>>>(qkv, kl, wz, conv_w, o, (int)np, heads, ks);
  return hipGetLastError();
}
hipError_t launch_transmil_head(const float* x, const float* w, const float* b, float* logits, int dim, int n_classes,
                                hipStream_t st) {
  transmil_head_kernel<<<1, 256, 0, st>>>(x, w, b, logits, dim, n_classes);
  return hipGetLastError();
}

hipError_t launch_transmil_assemble(const float* h, const float* cls, float* seq, int N, int rows, int dim, hipStream_t st) {
  const size_t n4 = (size_t)rows * (dim / 4);
  transmil_assemble_kernel<<<dim3((unsigned)((n4 + 255) / 256)), 256, 0, st>>>(h, cls, seq, N, rows, dim / 4);
  return hipGetLastError();
}
