// ln_partition.hip -- LayerNorm + zero-pad + region partition in one pass over the bag.
//
// Replaces: nn.LayerNorm (modules/rrt.py:121-123), the fp32 zero-pad torch.cat
// (modules/rmsa.py:199-200) and region_partition's permute+contiguous copy
// (modules/rmsa.py:28-39).  HBM-bound: reads L*D, writes Np*D floats, one wave per
// token row, float4 (16 B/lane) accesses, two-pass mean/variance held in registers.
#include "internal.h"

// FULL: dim == NV * 256 (every lane's columns exist) -> no lane predication in the row loops.  Not only a few
// instructions: the predicated form (v_cmp -> SGPR mask -> v_cndmask / s_and_saveexec around packed fp32 ops) gave
// wrong values in lanes 48..63 of a row now and then when the wave shared its SIMD with bf16-MFMA waves of another
// kernel (found as run-to-run differences of crmsa_logits_kernel next to rmsa_fused_x3_kernel)
template <int NV, bool FULL>   // float4 per lane: supports dim <= NV*256
__global__ __launch_bounds__(256) void ln_partition_kernel(const float* __restrict__ x,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ beta,
                                                           float* __restrict__ u, int dim, GridDev g,
                                                           int* __restrict__ zero, int n_zero) {
  if (zero != nullptr && blockIdx.x == 0)
    for (int i = threadIdx.x; i < n_zero; i += 256) zero[i] = 0;
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);   // padded-grid token index
  if (t >= g.Np) return;
  float* dst = u + (size_t)token_to_slot(t, g) * dim;
  if (t >= g.L) {   // pad row: exact zeros (they are NOT layer-normed in the reference)
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      int c = (v * 64 + lane) * 4;
      if (FULL || c < dim) *(float4*)(dst + c) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    return;
  }
  const float* src = x + (size_t)t * dim;
  float4 r[NV];
  float sum = 0.f;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    int c = (v * 64 + lane) * 4;
    r[v] = (FULL || c < dim) ? ld_row<NT_LN1>(src + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    sum += (r[v].x + r[v].y) + (r[v].z + r[v].w);
  }
  const float inv_d = 1.0f / (float)dim;
  const float mean = wave_sum(sum) * inv_d;
  float sq = 0.f;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    int c = (v * 64 + lane) * 4;
    if (FULL || c < dim) {
      float a = r[v].x - mean, b = r[v].y - mean, cc = r[v].z - mean, d = r[v].w - mean;
      sq += (a * a + b * b) + (cc * cc + d * d);
    }
  }
  const float rstd = 1.0f / sqrtf(wave_sum(sq) * inv_d + LN_EPS);
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    int c = (v * 64 + lane) * 4;
    if (FULL || c < dim) {
      float4 gm = *(const float4*)(gamma + c), bt = *(const float4*)(beta + c);
      float4 o;
      o.x = (r[v].x - mean) * rstd * gm.x + bt.x;
      o.y = (r[v].y - mean) * rstd * gm.y + bt.y;
      o.z = (r[v].z - mean) * rstd * gm.z + bt.z;
      o.w = (r[v].w - mean) * rstd * gm.w + bt.w;
      *(float4*)(dst + c) = o;
    }
  }
}

// Row-looping form (bags in flight): a FIXED grid of 4-wave blocks -- device CUs x `w` blocks, one wave per SIMD and block, so
// at w <= 2 the whole launch is resident at once even beside another bag's fused R-MSA block and sends the dispatcher no
// further waves -- wave gw takes the padded-grid tokens gw, gw + W, gw + 2 W, ... (W = waves of the launch).  gamma, beta and
// the grid constants are fetched once per wave (the one-wave-per-row form above spends 4 of its 6 float4 loads per lane on
// them), ahead of the first row's request (invariant loads behind it would drain the prefetch every trip).
// Row i + 1 is requested before row i is reduced; the request is unconditional (rows past the end, and pad rows, re-read the
// bag's last row and drop it).  The arithmetic of a row is ln_partition_kernel's, statement by statement: outputs are
// bit-identical (tests/test_rows_kernels_gpu.py).
// Resources (gfx950, kernel-resource-usage): <2, true> 49 VGPRs, 33 SGPRs, no LDS, no scratch (ln_partition_kernel<2, true>:
// 35 / 28) -- inside the 72 VGPRs that let two such waves sit beside two fused R-MSA waves of a SIMD.
// Measured (MI355X, default bench, four bags in flight): api.hip ROWS_W_DEFAULT, profiles/rows_in_flight_ab.txt.
template <int NV, bool FULL>
__device__ __forceinline__ void lnp_rows_request(const float* __restrict__ x, int t, int dim, int lane, float4 (&r)[NV]) {
  const float* src = x + (size_t)t * dim;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    int c = (v * 64 + lane) * 4;
    r[v] = (FULL || c < dim) ? ld_row<NT_LN1>(src + c) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}
// one padded-grid token t: statistics, normalisation and store of its row r (pad rows: zeros), as ln_partition_kernel
template <int NV, bool FULL>
__device__ __forceinline__ void lnp_rows_reduce(const float4 (&r)[NV], const float4 (&gm)[NV], const float4 (&bt)[NV],
                                                float* __restrict__ u, int t, int dim, int lane, float inv_d, const GridDev& g) {
  float* dst = u + (size_t)token_to_slot(t, g) * dim;
  if (t >= g.L) {   // pad row: exact zeros
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      int c = (v * 64 + lane) * 4;
      if (FULL || c < dim) *(float4*)(dst + c) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    return;
  }
  float sum = 0.f;
#pragma unroll
  for (int v = 0; v < NV; ++v) sum += (r[v].x + r[v].y) + (r[v].z + r[v].w);
  const float mean = wave_sum(sum) * inv_d;
  float sq = 0.f;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    int c = (v * 64 + lane) * 4;
    if (FULL || c < dim) {
      float a = r[v].x - mean, b = r[v].y - mean, cc = r[v].z - mean, d = r[v].w - mean;
      sq += (a * a + b * b) + (cc * cc + d * d);
    }
  }
  const float rstd = 1.0f / sqrtf(wave_sum(sq) * inv_d + LN_EPS);
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    int c = (v * 64 + lane) * 4;
    if (FULL || c < dim) {
      float4 o;
      o.x = (r[v].x - mean) * rstd * gm[v].x + bt[v].x;
      o.y = (r[v].y - mean) * rstd * gm[v].y + bt[v].y;
      o.z = (r[v].z - mean) * rstd * gm[v].z + bt[v].z;
      o.w = (r[v].w - mean) * rstd * gm[v].w + bt[v].w;
      *(float4*)(dst + c) = o;
    }
  }
}

template <int NV, bool FULL>
__global__ __launch_bounds__(256) void ln_partition_rows_kernel(const float* __restrict__ x,
                                                                const float* __restrict__ gamma,
                                                                const float* __restrict__ beta,
                                                                float* __restrict__ u, int dim, GridDev g,
                                                                int* __restrict__ zero, int n_zero) {
  if (zero != nullptr && blockIdx.x == 0)
    for (int i = threadIdx.x; i < n_zero; i += 256) zero[i] = 0;
  const int lane = threadIdx.x & 63;
  const int W = gridDim.x * 4;
  int t = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));   // padded-grid token index, wave-uniform
  if (t >= g.Np) return;
  float4 gm[NV], bt[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    int c = (v * 64 + lane) * 4;
    gm[v] = (FULL || c < dim) ? *(const float4*)(gamma + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    bt[v] = (FULL || c < dim) ? *(const float4*)(beta + c) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const float inv_d = 1.0f / (float)dim;
  const int last = g.L - 1;
  // two row buffers taking turns (a copy "row = next row" would wait for the request it was meant to leave in flight)
  float4 ra[NV], rb[NV];
  lnp_rows_request<NV, FULL>(x, t < g.L ? t : last, dim, lane, ra);
  for (;;) {
    const int tn = t + W;
    lnp_rows_request<NV, FULL>(x, tn < g.L ? tn : last, dim, lane, rb);
    __builtin_amdgcn_sched_barrier(0);                   // the next row's request is out before this row's first use waits
    lnp_rows_reduce<NV, FULL>(ra, gm, bt, u, t, dim, lane, inv_d, g);
    if (tn >= g.Np) break;
    t = tn + W;
    lnp_rows_request<NV, FULL>(x, t < g.L ? t : last, dim, lane, ra);
    __builtin_amdgcn_sched_barrier(0);
    lnp_rows_reduce<NV, FULL>(rb, gm, bt, u, tn, dim, lane, inv_d, g);
    if (t >= g.Np) break;
  }
}

// CUs of the current device, asked once per device (the row-looping kernels' grids are sized by it)
int device_cu_count() {
  static int cus[64] = {};
  int d = 0;
  (void)hipGetDevice(&d);
  d &= 63;
  if (cus[d] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess || n <= 0) n = 256;
    cus[d] = n;      // benign race: every thread stores the same number
  }
  return cus[d];
}

hipError_t launch_ln_partition(const float* x, const float* gamma, const float* beta, float* u,
                               int dim, const GridDev& g, hipStream_t st, int* zero, int n_zero, int rows_w) {
  if (rows_w > 0) {
    if (rows_w > ROWS_W_MAX) return hipErrorInvalidValue;
    const int rows_blocks = (g.Np + 3) / 4, fixed = device_cu_count() * rows_w;
    dim3 grid(rows_blocks < fixed ? rows_blocks : fixed), block(256);
#define RRT_LNP_ROWS(NV)                                                                         \
  do {                                                                                         \
    if (RRT_ALLOW_FULL && dim == NV * 256) ln_partition_rows_kernel<NV, true><<<grid, block, 0, st>>>(x, gamma, beta, u, dim, g, zero, n_zero);  \
    else ln_partition_rows_kernel<NV, false><<<grid, block, 0, st>>>(x, gamma, beta, u, dim, g, zero, n_zero);            \
  } while (0)
    if (dim <= 256) RRT_LNP_ROWS(1);
    else if (dim <= 512) RRT_LNP_ROWS(2);
    else if (dim <= 1024) RRT_LNP_ROWS(4);
    else RRT_LNP_ROWS(8);
#undef RRT_LNP_ROWS
    return hipGetLastError();
  }
  dim3 grid((g.Np + 3) / 4), block(256);
#define RRT_LNP(NV)                                                                              \
  do {                                                                                         \
    if (RRT_ALLOW_FULL && dim == NV * 256) ln_partition_kernel<NV, true><<<grid, block, 0, st>>>(x, gamma, beta, u, dim, g, zero, n_zero);  \
    else ln_partition_kernel<NV, false><<<grid, block, 0, st>>>(x, gamma, beta, u, dim, g, zero, n_zero);                 \
  } while (0)
  if (dim <= 256) RRT_LNP(1);
  else if (dim <= 512) RRT_LNP(2);
  else if (dim <= 1024) RRT_LNP(4);
  else RRT_LNP(8);
#undef RRT_LNP
  return hipGetLastError();
}
