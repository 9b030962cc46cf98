// region_attn_hd.hip -- the region attention forward of region_attn.hip at the other head dims: every multiple of 16 in
// [16, 256] except 64 (n_heads 2 / 4 / 16 / 32 at mlp_dim 512; the plug-in widths 256 / 384 / 768 / 1024 with 8 heads;
// CR-MSA's inner attention when its head dim qualifies).  fp32 data, exact-fp32 MFMA (v_mfma_f32_16x16x4_f32).
//
// Same mathematics as region_attn_kernel (identities (1) and (2) of region_attn.hip's header): q arrives scaled, the 1-D
// EPEG is a stencil over the query rows of the Q tile, the conv bias drops out, softmax(Q~ K^T) V is done flash-style and
// no [P, P] tensor exists beyond one run's scores in registers.
//   * block = (query group, head, region): nw <= NWMAX waves, a wave = one 16-query tile.  K and V of the (region, head)
//     stream through LDS in chunks of CK = 16 CT keys, staged once per block and shared by its waves; rows padded to
//     HD + 4 floats (the 16-slot XOR swizzle of the 64-wide kernel does not cover 48 / 96 / ... columns; with the pad 16
//     rows at one 16-byte slot land on 16 distinct bank groups at every head dim here, as in attn_bwd.hip's template).
//     A K | V chunk pair stays near 64 KB: two blocks per CU.
//   * scores TRANSPOSED (S^T = K Q~^T, A = K rows from LDS, B = the wave's Q~ fragments in registers: NF = HD / 16 float4
//     per lane), so lane (lr, lg) holds, for query lr, keys 4 lg + r of every 16-key tile: the row softmax needs two lane
//     swaps and P^T is already the A operand of P.V.  Key tiles are taken in runs of three (what is left of the region in
//     a run of two or one: nothing assumes P is a multiple of 16 or of the chunk), online softmax across runs.
//   * O: NF accumulators per lane.  Lane lr owns, of every 16 VW-column piece, columns VW lr .. VW lr + VW - 1 (VW = 4 / 2 / 1
//     as NF allows): the 16 lanes of a row read one contiguous run of V and write one contiguous run of o.
//   * Q~ fragments come straight from global memory (L2 / L1: the 16 + epeg_k - 1 rows a tile needs are shared by its lanes
//     and by the neighbouring tiles); rows outside [0, P) contribute nothing, also when epeg_k is wider than the region.
// No atomics, a fixed summation order: the same call twice gives the same bits.  Writes rows [0, n_regions P) of o, the
// head's columns of each, nothing else.
#include <type_traits>

#include "internal.h"

namespace {

constexpr float NEG_BIG = -3.0e38f;
constexpr float LOG2E = 1.4426950408889634f;

template <int HDT>
struct FwdCfg {
  static_assert(HDT % 16 == 0 && HDT >= 16 && HDT <= 256 && HDT != 64, "head dim");
  static constexpr int NF = HDT / 16;                 // float4 fragments (score side) = accumulators (apply side) per lane
  static constexpr int LDR = HDT + 4;                 // padded LDS row, floats
  static constexpr int CT = 512 / HDT > 9 ? 9 : 512 / HDT < 2 ? 2 : 512 / HDT;   // key tiles per chunk
  static constexpr int CK = 16 * CT;
  static constexpr int NWMAX = HDT <= 128 ? 8 : 4;    // waves (query tiles) per block
  // waves per SIMD the register budget is sized for (LDS holds two blocks per CU: 16 / 10-16 / 8 waves): 128 / 168 / 256 VGPRs
  static constexpr int WPE = HDT < 96 ? 4 : HDT <= 128 ? 3 : 2;
  static constexpr int VW = NF % 4 == 0 ? 4 : NF % 2 == 0 ? 2 : 1;   // apply-side piece width
  static constexpr size_t LDS = (size_t)2 * CK * LDR * sizeof(float);
  static_assert(LDS <= 80 * 1024, "two blocks per CU");
};

// s[u][r] = sum_d X[16 (t0 + u) + 4 lg + r][d] * f[query lr][d]   (u innermost: consecutive MFMAs hit different accumulators)
template <int HDT, int N>
__device__ __forceinline__ void hd_scores(const float* X, const float4 (&f)[HDT / 16], int lr, int lg, int t0, f32x4 (&s)[N]) {
  constexpr int LDR = FwdCfg<HDT>::LDR;
#pragma unroll
  for (int u = 0; u < N; ++u) s[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < HDT / 16; ++c) {
    float4 a[N];
#pragma unroll
    for (int u = 0; u < N; ++u) a[u] = *(const float4*)(X + ((t0 + u) * 16 + lr) * LDR + 4 * (4 * c + lg));
#pragma unroll
    for (int u = 0; u < N; ++u) s[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].x, f[c].x, s[u], 0, 0, 0);
#pragma unroll
    for (int u = 0; u < N; ++u) s[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].y, f[c].y, s[u], 0, 0, 0);
#pragma unroll
    for (int u = 0; u < N; ++u) s[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].z, f[c].z, s[u], 0, 0, 0);
#pragma unroll
    for (int u = 0; u < N; ++u) s[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].w, f[c].w, s[u], 0, 0, 0);
  }
}

// o[c][r'] += sum_{u, r} p[u][r] (query lr, key 16 (t0 + u) + 4 lg + r) * X[that key][column of accumulator c in lane lr]
// accumulator c = piece * VW + e  <->  column piece * 16 VW + VW lr + e
template <int HDT, int N>
__device__ __forceinline__ void hd_apply(const float* X, const f32x4 (&p)[N], int lr, int lg, int t0, f32x4 (&o)[HDT / 16]) {
  constexpr int NF = HDT / 16, LDR = FwdCfg<HDT>::LDR, VW = FwdCfg<HDT>::VW;
#pragma unroll
  for (int u = 0; u < N; ++u)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float* src = X + ((t0 + u) * 16 + 4 * lg + r) * LDR + VW * lr;
      const float w = p[u][r];
#pragma unroll
      for (int c = 0; c < NF; c += VW) {
        if constexpr (VW == 4) {
          const float4 v = *(const float4*)(src + 16 * c);
          o[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(w, v.x, o[c], 0, 0, 0);
          o[c + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w, v.y, o[c + 1], 0, 0, 0);
          o[c + 2] = __builtin_amdgcn_mfma_f32_16x16x4f32(w, v.z, o[c + 2], 0, 0, 0);
          o[c + 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(w, v.w, o[c + 3], 0, 0, 0);
        } else if constexpr (VW == 2) {
          const float2 v = *(const float2*)(src + 16 * c);
          o[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(w, v.x, o[c], 0, 0, 0);
          o[c + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w, v.y, o[c + 1], 0, 0, 0);
        } else {
          o[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(w, src[16 * c], o[c], 0, 0, 0);
        }
      }
    }
}

// rows [r0, r0 + nrows) of K and of V (head columns) -> the padded LDS chunk pair; rows >= P: zeros.
// Four (K, V) slot pairs per thread and trip: eight 16-byte loads in flight.
template <int HDT>
__device__ __forceinline__ void hd_stage(float* Ks, float* Vs, const float* kbase, const float* vbase, int ld, int r0,
                                         int nrows, int P, int tid, int nth) {
  constexpr int SL = HDT / 4, LDR = FwdCfg<HDT>::LDR;
  const int total = nrows * SL;
  for (int base = tid; base < total; base += 4 * nth) {
    float4 k4[4], v4[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int idx = base + u * nth;
      const int m = idx / SL, s = idx - m * SL;
      const bool ok = idx < total && r0 + m < P;
      const size_t off = (size_t)(r0 + m) * ld + 4 * s;
      k4[u] = ok ? *(const float4*)(kbase + off) : make_float4(0.f, 0.f, 0.f, 0.f);
      v4[u] = ok ? *(const float4*)(vbase + off) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int idx = base + u * nth;
      const int m = idx / SL, s = idx - m * SL;
      if (idx < total) {
        *(float4*)(Ks + m * LDR + 4 * s) = k4[u];
        *(float4*)(Vs + m * LDR + 4 * s) = v4[u];
      }
    }
  }
}

// grid (query groups, heads, regions), block = nw waves (nw <= NWMAX, chosen by the launcher so that no wave idles)
template <int HDT>
__global__ __launch_bounds__(FwdCfg<HDT>::NWMAX * 64, FwdCfg<HDT>::WPE) void region_attn_hd_kernel(
    const float* __restrict__ qkv, const float* __restrict__ pe_w, float* __restrict__ o, int P, int dim, int epeg_k) {
  using C = FwdCfg<HDT>;
  constexpr int NF = C::NF, CT = C::CT, CK = C::CK, VW = C::VW;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Ks = (float*)smem;
  float* Vs = Ks + CK * C::LDR;
  const int tid = threadIdx.x, lane = tid & 63, nth = blockDim.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nw = __builtin_amdgcn_readfirstlane(nth >> 6);
  const int lr = lane & 15, lg = lane >> 4;
  const int head = blockIdx.y, reg = blockIdx.z;
  const int ld = 3 * dim;
  const size_t row0 = (size_t)reg * P;
  const float* qbase = qkv + row0 * ld + head * HDT;
  const float* kbase = qbase + dim;
  const float* vbase = qbase + 2 * dim;
  const int i0 = (blockIdx.x * nw + wave) * 16;           // first query of this wave
  const bool active = i0 < P;
  const int m = i0 + lr;

  // ---- Q~ fragments (B operand of S^T): fq[c] = log2(e) * Q~[m][16 c + 4 lg .. + 3] ----
  float4 fq[NF];
#pragma unroll
  for (int c = 0; c < NF; ++c) fq[c] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (active) {
    if (m < P) {
#pragma unroll
      for (int c = 0; c < NF; ++c) fq[c] = *(const float4*)(qbase + (size_t)m * ld + 4 * (4 * c + lg));
    }
    if (epeg_k > 0) {
      const float* w = pe_w + head * epeg_k;
      const int half = epeg_k >> 1;
      // TU taps per trip: TU * NF independent 16-byte loads in flight (one tap at a time is a chain of L2 round trips at
      // the small head dims); the taps are still added in order
      constexpr int TU = NF >= 16 ? 1 : NF >= 8 ? 2 : 4;
      for (int t = 0; t < epeg_k; t += TU) {
        float4 v[TU][NF];
        float wt[TU];
#pragma unroll
        for (int u = 0; u < TU; ++u) {
          const int r = m + t + u - half;
          const bool ok = t + u < epeg_k && m < P && r >= 0 && r < P;
          wt[u] = t + u < epeg_k ? w[t + u] : 0.f;
#pragma unroll
          for (int c = 0; c < NF; ++c)
            v[u][c] = ok ? *(const float4*)(qbase + (size_t)r * ld + 4 * (4 * c + lg)) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < TU; ++u)
#pragma unroll
          for (int c = 0; c < NF; ++c) {
            fq[c].x += wt[u] * v[u][c].x; fq[c].y += wt[u] * v[u][c].y; fq[c].z += wt[u] * v[u][c].z; fq[c].w += wt[u] * v[u][c].w;
          }
      }
    }
#pragma unroll
    for (int c = 0; c < NF; ++c) {   // scores in log2 units: softmax via exp2
      fq[c].x *= LOG2E; fq[c].y *= LOG2E; fq[c].z *= LOG2E; fq[c].w *= LOG2E;
    }
  }

  float m_run = NEG_BIG, l_run = 0.f;
  bool first = true;
  f32x4 oacc[NF];
#pragma unroll
  for (int c = 0; c < NF; ++c) oacc[c] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int r0 = 0; r0 < P; r0 += CK) {
    const int nt = min(CT, (P - r0 + 15) >> 4);            // key tiles of this chunk that hold a key of the region
    if (r0 > 0) __syncthreads();
    hd_stage<HDT>(Ks, Vs, kbase, vbase, ld, r0, nt * 16, P, tid, nth);
    __syncthreads();
    if (!active) continue;
    // one run of N key tiles: S^T, mask, online softmax, O += P V
    auto run = [&](auto nc, const int t0) {
      constexpr int N = decltype(nc)::value;
      f32x4 s[N];
      hd_scores<HDT, N>(Ks, fq, lr, lg, t0, s);
      const int j0 = r0 + t0 * 16;
      if (j0 + 16 * N > P) {   // the region's last run only: mask keys >= P
#pragma unroll
        for (int u = 0; u < N; ++u)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (j0 + u * 16 + 4 * lg + r >= P) s[u][r] = NEG_BIG;
      }
      float cmax = NEG_BIG;
#pragma unroll
      for (int u = 0; u < N; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) cmax = fmaxf(cmax, s[u][r]);
      cmax = max_xor32(max_xor16(cmax));
      const float m_new = fmaxf(m_run, cmax);
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      m_run = m_new;
      float psum = 0.f;
#pragma unroll
      for (int u = 0; u < N; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = __builtin_amdgcn_exp2f(s[u][r] - m_new);
          s[u][r] = p;
          psum += p;
        }
      l_run = l_run * alpha + psum;   // per-lane partial (this lane's keys); the lanes of a query share alpha
      if (!first) {
        // rescale O: row r' of the O tile is query 4 lg + r', whose alpha lives in lane 4 lg + r'
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float ar = __shfl(alpha, 4 * lg + r);
#pragma unroll
          for (int c = 0; c < NF; ++c) oacc[c][r] *= ar;
        }
      }
      first = false;
      hd_apply<HDT, N>(Vs, s, lr, lg, t0, oacc);
    };
    int t0 = 0;
    for (; t0 + 3 <= nt; t0 += 3) run(std::integral_constant<int, 3>{}, t0);
    if (nt - t0 == 2) run(std::integral_constant<int, 2>{}, t0);
    else if (nt - t0 == 1) run(std::integral_constant<int, 1>{}, t0);
  }
  if (!active) return;
  const float inv = 1.0f / sum_xor32(sum_xor16(l_run));
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float ir = __shfl(inv, 4 * lg + r);
    const int i = i0 + 4 * lg + r;
    if (i < P) {
      float* dst = o + (row0 + i) * dim + head * HDT + VW * lr;
#pragma unroll
      for (int c = 0; c < NF; c += VW) {
        if constexpr (VW == 4)
          *(float4*)(dst + 16 * c) = make_float4(oacc[c][r] * ir, oacc[c + 1][r] * ir, oacc[c + 2][r] * ir, oacc[c + 3][r] * ir);
        else if constexpr (VW == 2)
          *(float2*)(dst + 16 * c) = make_float2(oacc[c][r] * ir, oacc[c + 1][r] * ir);
        else
          dst[16 * c] = oacc[c][r] * ir;
      }
    }
  }
}

template <int HDT>
hipError_t launch_hd(const float* qkv, const float* pe_w, float* o, int n_regions, int P, int dim, int heads, int epeg_k,
                     hipStream_t st) {
  using C = FwdCfg<HDT>;
  const int ntiles = (P + 15) / 16;
  const int groups = (ntiles + C::NWMAX - 1) / C::NWMAX;
  const int nw = (ntiles + groups - 1) / groups;            // even split: 9 tiles -> 5 + 4 (NWMAX 8), 3 x 3 (NWMAX 4)
  static OncePerDevice once;
  if (C::LDS > 64 * 1024 && once.first())
    (void)hipFuncSetAttribute((const void*)region_attn_hd_kernel<HDT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)C::LDS);
  region_attn_hd_kernel<HDT><<<dim3(groups, heads, n_regions), nw * 64, C::LDS, st>>>(qkv, pe_w, o, P, dim, epeg_k);
  return hipGetLastError();
}

}  // namespace

bool region_attention_hd_supported(int P, int dim, int heads, int epeg_k) {
  if (P < 1 || dim < 1 || heads < 1 || dim % heads) return false;
  const int hd = dim / heads;
  return hd % 16 == 0 && hd >= 16 && hd <= 256 && hd != 64 && epeg_k <= 63;
}

hipError_t launch_region_attention_hd(const float* qkv, const float* pe_w, float* o, int n_regions, int P, int dim,
                                      int heads, int epeg_k, hipStream_t st) {
  if (pe_w == nullptr || epeg_k < 0) epeg_k = 0;
  if (!region_attention_hd_supported(P, dim, heads, epeg_k) || n_regions < 1 || n_regions > 65535 || heads > 65535)
    return hipErrorInvalidValue;
  switch (dim / heads) {
#define RRT_HD_CASE(H) case H: return launch_hd<H>(qkv, pe_w, o, n_regions, P, dim, heads, epeg_k, st)
    RRT_HD_CASE(16); RRT_HD_CASE(32); RRT_HD_CASE(48); RRT_HD_CASE(80); RRT_HD_CASE(96); RRT_HD_CASE(112);
    RRT_HD_CASE(128); RRT_HD_CASE(144); RRT_HD_CASE(160); RRT_HD_CASE(176); RRT_HD_CASE(192); RRT_HD_CASE(208);
    RRT_HD_CASE(224); RRT_HD_CASE(240); RRT_HD_CASE(256);
#undef RRT_HD_CASE
  }
  return hipErrorInvalidValue;
}
