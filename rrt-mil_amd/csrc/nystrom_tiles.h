// nystrom_tiles.h -- the tile helpers shared by nystrom.hip (forward) and nystrom_bwd.hip (backward).  Every block is
// 256 threads = 4 waves; a wave owns 16 rows x 64 columns of the block's 64 x 64 tile (four 16 x 16 MFMA accumulators).
// Operand tiles go through LDS: A as [row][k] with a row stride of 4 (mod 32) floats, B as [k][column] with a row stride of
// 16 (mod 64) floats, so that the 64 lanes of one operand read hit 64 different banks.
#pragma once
#include "internal.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int NM = 256;        // landmarks
constexpr int ND = 64;         // head dim
constexpr int LDA = 68;        // LDS row stride of an A tile with 64 k-columns
constexpr int LDB = 80;        // LDS row stride of a B tile with 64 columns

// acc (this wave's 16 rows x 64 columns) += As[16][K] . Bs[K][64].  16x16x4: lane l holds A[l & 15][l >> 4] and
// B[l >> 4][l & 15]; result register r of lane l is C[4 (l >> 4) + r][l & 15].
template <int NJ = 4>
__device__ __forceinline__ void mma_16x64(const float* As, int lda, const float* Bs, int ldb, int K, f32x4 (&acc)[NJ]) {
  const int lane = threadIdx.x & 63, r = lane & 15, kq = lane >> 4;
  for (int k0 = 0; k0 < K; k0 += 4) {
    const float a = As[r * lda + k0 + kq];
    const float* bp = Bs + (k0 + kq) * ldb + r;
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bp[16 * j], acc[j], 0, 0, 0);
  }
}

// dst[r][c] <- src[r * src_ld + c], rows x 64 floats, by the whole block
__device__ __forceinline__ void stage_rows(float* dst, int ld, const float* __restrict__ src, size_t src_ld, int rows) {
  for (int i = threadIdx.x; i < rows * 16; i += 256) {
    const int r = i >> 4, c = (i & 15) * 4;
    *(float4*)(dst + r * ld + c) = *(const float4*)(src + (size_t)r * src_ld + c);
  }
}
// dst[c][r] <- src[r * src_ld + c], 64 x 64 (the B operand of a product with a transposed right factor)
__device__ __forceinline__ void stage_64x64_t(float* dst, int ld, const float* __restrict__ src, size_t src_ld) {
  for (int i = threadIdx.x; i < 64 * 16; i += 256) {
    const int r = i & 63, c = (i >> 6) * 4;
    const float4 v = *(const float4*)(src + (size_t)r * src_ld + c);
    dst[(c + 0) * ld + r] = v.x;
    dst[(c + 1) * ld + r] = v.y;
    dst[(c + 2) * ld + r] = v.z;
    dst[(c + 3) * ld + r] = v.w;
  }
}

// reductions over the 16 lanes that share a row of the accumulator layout
__device__ __forceinline__ float row16_max(float v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float row16_sum(float v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o);
  return v;
}

// scores of this block's 64 rows (As, staged by the caller) against the 256 landmarks kl_h, and their row softmax:
// on return s[ct][j][r] is the probability of row 16 w + 4 (lane >> 4) + r, column 64 ct + 16 j + (lane & 15)
__device__ __forceinline__ void scores_softmax_256(const float* As, float* Bs, const float* __restrict__ kl_h, f32x4 (&s)[4][4]) {
  const int w = threadIdx.x >> 6;
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    __syncthreads();
    stage_64x64_t(Bs, LDB, kl_h + (size_t)ct * 64 * ND, ND);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) s[ct][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    mma_16x64(As + w * 16 * LDA, LDA, Bs, LDB, ND, s[ct]);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float m = -INFINITY;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int j = 0; j < 4; ++j) m = fmaxf(m, s[ct][j][r]);
    m = row16_max(m);
    float sum = 0.f;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float p = expf(s[ct][j][r] - m);
        s[ct][j][r] = p;
        sum += p;
      }
    sum = row16_sum(sum);
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int j = 0; j < 4; ++j) s[ct][j][r] = s[ct][j][r] / sum;
  }
}

}  // namespace
