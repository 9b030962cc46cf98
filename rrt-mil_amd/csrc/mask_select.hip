// mask_select.hip -- MHIM-MIL's hard-instance mask selection on the device, and the row movement around it
// (include/rrt_hip.h: rrt_mask_select_f32, rrt_gather_rows_f32, rrt_scatter_rows_f32; host side: api_mask.hip).
//
// Selection = four plain launches, nothing handed over between blocks inside a launch:
//   1. mask_rank_kernel   a counting rank.  The n scores become 32-bit keys whose UNSIGNED order is the order the ABI defines
//                         (-0 folded onto +0, every NaN onto the one greatest key), and token i counts, over all j,
//                             asc  = #{j : key_j < key_i} + #{j < i : key_j == key_i}   its place in ascending order
//                             desc = #{j : key_j > key_i} + #{j < i : key_j == key_i}   its place in descending order
//                         -- "equal values: lower index first" IS the second term, so no tie needs a second look.  The j range
//                         is tiled through LDS (every lane reads the same key: a broadcast ds_read_b128 per four keys) and cut
//                         into `split` chunks on blockIdx.y so that a 9 000-token bag still fills the chip; a chunk's counts go
//                         to its own row of part_asc / part_desc [split, n] (integers: any order of summation is the same sum).
//                         Away from the diagonal tile the index term needs no compare: a tile wholly below the block's tokens
//                         counts key_j <= key_i, one wholly above counts key_j < key_i -- two VALU instructions (a compare and
//                         an add with carry-in) per pair and per order.  Only the orders some stage reads are counted.
//   2. mask_flag_kernel   sums a token's partial ranks, tests every stage (rank < k and pick[rank] != 0), writes kept [n], the
//                         optional mask and the block's kept count.
//   3. mask_scan_kernel   ONE block: exclusive scan of the <= 1024 block counts; count[0] = the total.
//   4. mask_place_kernel  ids[0:count) = kept ascending, ids[count:n) = the others ascending (a kept token's place is its
//                         block's offset + its prefix inside the block; a dropped token i sits at count + i - kept-before-i).
// Same inputs, same bits: integer arithmetic and fixed places only, no atomics.
//
// Vote fusion over heads (rrt_mask_select_vote_f32, a [heads, n]) = six plain launches under the same rules:
//   1. mask_rank_heads_kernel  the counting rank above with the head on blockIdx.z: parts [heads, split, n].
//   2. mask_vote_kernel        vote[s, i] = the number of heads that hold token i among their first k_s (a byte, 0..heads), and
//                              per block and stage the histogram of the heads + 1 vote values (wave ballots, summed in LDS).
//   3. mask_vote_scan_kernel   one block per (stage, vote value): exclusive scan of that value's <= 1024 block counts and its total.
//   4. mask_vote_flag_kernel   the fused order is "vote descending, lower index first": its keys are small integers, so a token's
//                              place is (tokens of a greater vote) + (its vote in earlier blocks) + (its ballot prefix among the
//                              equal votes of its block) -- no second O(n^2) pass.  Then mask_flag_kernel's test and outputs.
//   5. / 6. mask_scan_kernel, mask_place_kernel as above.
#include "internal.h"

namespace {
constexpr int MS_BLOCK = 256;      // tokens per block, threads per block, and the LDS sub-tile the order relation is decided on
constexpr int MS_TILE = 1024;      // keys per LDS fill
constexpr unsigned MS_KEY_NAN = 0xFFFFFFFFu;

__device__ __forceinline__ unsigned order_key(float v) {
  if (v != v) return MS_KEY_NAN;                       // NaN: greater than every number, all NaNs equal
  unsigned b = __float_as_uint(v);
  if (b == 0x80000000u) b = 0u;                        // -0.0 == +0.0
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);   // (+inf -> 0xFF800000 < MS_KEY_NAN)
}

// REL: where the sub-tile's tokens lie relative to this block's: -1 all lower indices, +1 all higher, 0 the block's own
// (`li` = this thread's place inside it).  cnt: valid keys of the sub-tile (256 but for the bag's last one).
template <int REL, bool ASC, bool DESC>
__device__ __forceinline__ void count_tile(const unsigned* t, int cnt, unsigned ki, int li, unsigned& asc, unsigned& desc) {
  auto one = [&](unsigned kj, int j) {
    if constexpr (REL < 0) {
      if constexpr (ASC) asc += kj <= ki;
      if constexpr (DESC) desc += kj >= ki;
    } else if constexpr (REL > 0) {
      if constexpr (ASC) asc += kj < ki;
      if constexpr (DESC) desc += kj > ki;
    } else {
      const bool tie = (kj == ki) & (j < li);
      if constexpr (ASC) asc += (kj < ki) | tie;
      if constexpr (DESC) desc += (kj > ki) | tie;
    }
  };
  const int c4 = cnt & ~3;
#pragma unroll 4
  for (int j = 0; j < c4; j += 4) {
    const uint4 k4 = *(const uint4*)(t + j);
    one(k4.x, j);
    one(k4.y, j + 1);
    one(k4.z, j + 2);
    one(k4.w, j + 3);
  }
  for (int j = c4; j < cnt; ++j) one(t[j], j);
}

// one block's 256 tokens against one chunk of the j range (the body of both rank kernels)
template <bool ASC, bool DESC>
__device__ __forceinline__ void rank_block(const float* __restrict__ a, int n, int chunk_len, unsigned* __restrict__ part_asc,
                                           unsigned* __restrict__ part_desc, unsigned* tile /* LDS [MS_TILE], 16-byte aligned */) {
  const int i0 = blockIdx.x * MS_BLOCK, i = i0 + threadIdx.x;
  const unsigned ki = i < n ? order_key(a[i]) : 0u;
  const int j_begin = blockIdx.y * chunk_len, j_end = min(n, j_begin + chunk_len);
  unsigned asc = 0, desc = 0;
  for (int j0 = j_begin; j0 < j_end; j0 += MS_TILE) {
    __syncthreads();
    for (int t = threadIdx.x; t < MS_TILE; t += MS_BLOCK) {
      const int j = j0 + t;
      tile[t] = j < j_end ? order_key(a[j]) : 0u;      // (beyond j_end: never counted, cnt below stops in front of it)
    }
    __syncthreads();
    for (int s0 = 0; s0 < MS_TILE && j0 + s0 < j_end; s0 += MS_BLOCK) {      // block-uniform
      const int js = j0 + s0, cnt = min(MS_BLOCK, j_end - js);
      if (js < i0) count_tile<-1, ASC, DESC>(tile + s0, cnt, ki, 0, asc, desc);
      else if (js > i0) count_tile<1, ASC, DESC>(tile + s0, cnt, ki, 0, asc, desc);
      else count_tile<0, ASC, DESC>(tile + s0, cnt, ki, (int)threadIdx.x, asc, desc);
    }
  }
  if (i < n) {
    if constexpr (ASC) part_asc[(size_t)blockIdx.y * n + i] = asc;
    if constexpr (DESC) part_desc[(size_t)blockIdx.y * n + i] = desc;
  }
}

template <bool ASC, bool DESC>
__global__ __launch_bounds__(MS_BLOCK) void mask_rank_kernel(const float* __restrict__ a, int n, int chunk_len,
                                                             unsigned* __restrict__ part_asc, unsigned* __restrict__ part_desc) {
  __shared__ __attribute__((aligned(16))) unsigned tile[MS_TILE];
  rank_block<ASC, DESC>(a, n, chunk_len, part_asc, part_desc, tile);
}

// the block's exclusive prefix of `flag` over its 256 threads (4 waves) and the block total, through ballots
__device__ __forceinline__ int block_prefix(bool flag, int* wave_tot /* LDS [4] */, int& total) {
  const unsigned long long b = __ballot(flag);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int in_wave = __popcll(b & ((1ull << lane) - 1ull));
  if (lane == 0) wave_tot[w] = __popcll(b);
  __syncthreads();
  int before = 0;
  total = 0;
#pragma unroll
  for (int v = 0; v < MS_BLOCK / 64; ++v) {
    const int c = wave_tot[v];
    before += v < w ? c : 0;
    total += c;
  }
  return before + in_wave;
}

__global__ __launch_bounds__(MS_BLOCK) void mask_flag_kernel(const unsigned* __restrict__ part_asc, const unsigned* __restrict__ part_desc,
                                                             int n, int split, MaskStages st, int invert,
                                                             unsigned char* __restrict__ kept, unsigned char* __restrict__ mask,
                                                             int* __restrict__ block_cnt) {
  __shared__ int wave_tot[MS_BLOCK / 64];
  const int i = blockIdx.x * MS_BLOCK + threadIdx.x;
  bool keep = false;
  if (i < n) {
    unsigned asc = 0, desc = 0;
    for (int s = 0; s < split; ++s) {
      if (st.any_asc) asc += part_asc[(size_t)s * n + i];
      if (st.any_desc) desc += part_desc[(size_t)s * n + i];
    }
    bool sel = false;
    for (int s = 0; s < st.n; ++s) {
      const unsigned r = st.largest[s] ? desc : asc;
      if (r < (unsigned)st.k[s]) sel |= st.pick[s] == nullptr || st.pick[s][r] != 0;
    }
    keep = invert ? sel : !sel;
    kept[i] = keep;
    if (mask) mask[i] = !keep;
  }
  int total;
  block_prefix(keep, wave_tot, total);
  if (threadIdx.x == 0) block_cnt[blockIdx.x] = total;
}

// one block of 1024 threads over nb <= 1024 block counts
__global__ __launch_bounds__(1024) void mask_scan_kernel(const int* __restrict__ block_cnt, int nb, int* __restrict__ block_off,
                                                         long long* __restrict__ count) {
  __shared__ int s[1024];
  const int t = threadIdx.x;
  const int own = t < nb ? block_cnt[t] : 0;
  s[t] = own;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const int v = t >= d ? s[t - d] : 0;
    __syncthreads();
    s[t] += v;
    __syncthreads();
  }
  if (t < nb) block_off[t] = s[t] - own;
  if (t == 1023) count[0] = s[1023];
}

__global__ __launch_bounds__(MS_BLOCK) void mask_place_kernel(const unsigned char* __restrict__ kept, int n,
                                                              const int* __restrict__ block_off,
                                                              const long long* __restrict__ count, long long* __restrict__ ids) {
  __shared__ int wave_tot[MS_BLOCK / 64];
  const int i = blockIdx.x * MS_BLOCK + threadIdx.x;
  const bool keep = i < n && kept[i] != 0;
  int total;
  const int before = block_off[blockIdx.x] + block_prefix(keep, wave_tot, total);     // kept tokens in front of i
  if (i < n) {
    const long long at = keep ? (long long)before : count[0] + (long long)(i - before);
    if (at >= 0 && at < n) ids[at] = i;      // (always true: count <= n and before <= i; the guard costs nothing)
  }
}

// ---- multi-head vote fusion (rrt_mask_select_vote_f32): the rank per head, then the fused order from small integer keys
// the counting rank with the head on blockIdx.z: head h reads a[h, :], writes rows [h * split, (h + 1) * split) of the parts
template <bool ASC, bool DESC>
__global__ __launch_bounds__(MS_BLOCK) void mask_rank_heads_kernel(const float* __restrict__ a, int n, int chunk_len,
                                                                   unsigned* __restrict__ part_asc, unsigned* __restrict__ part_desc) {
  __shared__ __attribute__((aligned(16))) unsigned tile[MS_TILE];
  const size_t h = blockIdx.z, rows = (size_t)h * gridDim.y * n;
  rank_block<ASC, DESC>(a + h * n, n, chunk_len, part_asc + rows, part_desc + rows, tile);
}

// per wave, the number of lanes whose vote is v, for every v in 0..heads: cnt [waves][MASK_VOTE_VALUES] in LDS; returns the
// lane's prefix among the equal votes of its own wave.  (vote < 0: the lane takes no part.)
__device__ __forceinline__ int vote_wave_counts(int vote, int heads, int* cnt /* LDS [MS_BLOCK / 64][MASK_VOTE_VALUES] */) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int mine = 0;
  for (int v = 0; v <= heads; ++v) {                            // block-uniform trip count
    const unsigned long long b = __ballot(vote == v);
    if (vote == v) mine = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) cnt[w * MASK_VOTE_VALUES + v] = __popcll(b);
  }
  return mine;
}

// vote[s, i] = #{heads h : rank_h(i) < k_s} in stage s's order, and the block's histogram of the heads + 1 vote values per stage:
// hist [(s * MASK_VOTE_VALUES + v) * blocks + block]
__global__ __launch_bounds__(MS_BLOCK) void mask_vote_kernel(const unsigned* __restrict__ part_asc, const unsigned* __restrict__ part_desc,
                                                             int n, int split, int heads, MaskStages st,
                                                             unsigned char* __restrict__ vote, int* __restrict__ hist) {
  __shared__ int cnt[3][MS_BLOCK / 64][MASK_VOTE_VALUES];
  const int i = blockIdx.x * MS_BLOCK + threadIdx.x;
  int votes[3] = {-1, -1, -1};
  if (i < n) {
    for (int s = 0; s < st.n; ++s) votes[s] = 0;
    for (int h = 0; h < heads; ++h) {
      unsigned asc = 0, desc = 0;
      for (int c = 0; c < split; ++c) {
        const size_t at = ((size_t)h * split + c) * n + i;
        if (st.any_asc) asc += part_asc[at];
        if (st.any_desc) desc += part_desc[at];
      }
      for (int s = 0; s < st.n; ++s) votes[s] += (st.largest[s] ? desc : asc) < (unsigned)st.k[s];
    }
    for (int s = 0; s < st.n; ++s) vote[(size_t)s * n + i] = (unsigned char)votes[s];
  }
  for (int s = 0; s < st.n; ++s) vote_wave_counts(votes[s], heads, &cnt[s][0][0]);
  __syncthreads();
  for (int e = threadIdx.x; e < st.n * MASK_VOTE_VALUES; e += MS_BLOCK) {
    const int s = e / MASK_VOTE_VALUES, v = e - s * MASK_VOTE_VALUES;
    if (v <= heads) {
      int t = 0;
      for (int w = 0; w < MS_BLOCK / 64; ++w) t += cnt[s][w][v];
      hist[(size_t)e * gridDim.x + blockIdx.x] = t;
    }
  }
}

// block (s, v) of n_stages * (heads + 1): exclusive scan over the nb <= 1024 blocks' counts of vote value v in stage s ->
// off [(s * MASK_VOTE_VALUES + v) * nb + block], tot [s * MASK_VOTE_VALUES + v]
__global__ __launch_bounds__(1024) void mask_vote_scan_kernel(const int* __restrict__ hist, int nb, int heads, int* __restrict__ off,
                                                              int* __restrict__ tot) {
  __shared__ int s[1024];
  const int t = threadIdx.x;
  const int e = (blockIdx.x / (heads + 1)) * MASK_VOTE_VALUES + blockIdx.x % (heads + 1);
  const int own = t < nb ? hist[(size_t)e * nb + t] : 0;
  s[t] = own;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const int v = t >= d ? s[t - d] : 0;
    __syncthreads();
    s[t] += v;
    __syncthreads();
  }
  if (t < nb) off[(size_t)e * nb + t] = s[t] - own;
  if (t == 1023) tot[e] = s[1023];
}

// a token's place in stage s's fused order (vote descending, equal votes: lower index first) =
//   #{tokens of a greater vote} + #{tokens of its vote in earlier blocks} + its prefix among the equal votes of its block;
// then mask_flag_kernel's test and outputs
__global__ __launch_bounds__(MS_BLOCK) void mask_vote_flag_kernel(const unsigned char* __restrict__ vote, const int* __restrict__ off,
                                                                  const int* __restrict__ tot, int n, int heads, MaskStages st,
                                                                  int invert, unsigned char* __restrict__ kept,
                                                                  unsigned char* __restrict__ mask, int* __restrict__ block_cnt) {
  __shared__ int cnt[3][MS_BLOCK / 64][MASK_VOTE_VALUES];
  __shared__ int base[3][MASK_VOTE_VALUES];
  __shared__ int wave_tot[MS_BLOCK / 64];
  const int i = blockIdx.x * MS_BLOCK + threadIdx.x, w = threadIdx.x >> 6;
  for (int e = threadIdx.x; e < st.n * MASK_VOTE_VALUES; e += MS_BLOCK) {
    const int s = e / MASK_VOTE_VALUES, v = e - s * MASK_VOTE_VALUES;
    int above = 0;
    for (int u = v + 1; u <= heads; ++u) above += tot[s * MASK_VOTE_VALUES + u];
    base[s][v] = above;
  }
  int votes[3] = {-1, -1, -1}, in_wave[3] = {0, 0, 0};
  for (int s = 0; s < st.n; ++s) {
    if (i < n) votes[s] = min((int)vote[(size_t)s * n + i], heads);
    in_wave[s] = vote_wave_counts(votes[s], heads, &cnt[s][0][0]);
  }
  __syncthreads();
  bool keep = false;
  if (i < n) {
    bool sel = false;
    for (int s = 0; s < st.n; ++s) {
      const int v = votes[s];
      int pos = base[s][v] + off[((size_t)s * MASK_VOTE_VALUES + v) * gridDim.x + blockIdx.x] + in_wave[s];
      for (int u = 0; u < w; ++u) pos += cnt[s][u][v];
      if (pos >= 0 && pos < st.k[s]) sel |= st.pick[s] == nullptr || st.pick[s][pos] != 0;
    }
    keep = invert ? sel : !sel;
    kept[i] = keep;
    if (mask) mask[i] = !keep;
  }
  int total;
  block_prefix(keep, wave_tot, total);
  if (threadIdx.x == 0) block_cnt[blockIdx.x] = total;
}

// ---- rows by index
constexpr int ROWS_BLOCK = 256;

__global__ __launch_bounds__(ROWS_BLOCK) void gather_rows_kernel(const float* __restrict__ src, const long long* __restrict__ ids,
                                                                 float* __restrict__ dst, long long n_rows, long long n_src, int dim4) {
  const long long total = n_rows * dim4;
  const float qnan = __uint_as_float(0x7FC00000u);
  for (long long e = (long long)blockIdx.x * ROWS_BLOCK + threadIdx.x; e < total; e += (long long)gridDim.x * ROWS_BLOCK) {
    const long long r = e / dim4;
    const int c = (int)(e - r * dim4);
    const long long id = ids[r];
    float4 v = make_float4(qnan, qnan, qnan, qnan);
    if (id >= 0 && id < n_src) v = *(const float4*)(src + (id * dim4 + c) * 4);
    *(float4*)(dst + e * 4) = v;
  }
}

__global__ __launch_bounds__(ROWS_BLOCK) void scatter_rows_kernel(const float* __restrict__ src, const long long* __restrict__ ids,
                                                                  float* __restrict__ dst, long long n_rows, long long n_dst, int dim4) {
  const long long total = n_rows * dim4;
  for (long long e = (long long)blockIdx.x * ROWS_BLOCK + threadIdx.x; e < total; e += (long long)gridDim.x * ROWS_BLOCK) {
    const long long r = e / dim4;
    const int c = (int)(e - r * dim4);
    const long long id = ids[r];
    if (id >= 0 && id < n_dst) *(float4*)(dst + (id * dim4 + c) * 4) = *(const float4*)(src + e * 4);
  }
}

int rows_grid(long long total) {
  const long long b = (total + ROWS_BLOCK - 1) / ROWS_BLOCK;
  return (int)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}
}  // namespace

MaskSplit mask_select_split(int n) {
  const int tb = (n + MS_BLOCK - 1) / MS_BLOCK;
  int s = 1024 / tb;
  s = s < 1 ? 1 : (s > MASK_SPLIT_MAX ? MASK_SPLIT_MAX : s);
  MaskSplit m;
  m.chunk_len = ((n + s - 1) / s + MS_BLOCK - 1) / MS_BLOCK * MS_BLOCK;
  m.split = (n + m.chunk_len - 1) / m.chunk_len;
  m.blocks = tb;
  return m;
}

hipError_t launch_mask_select(const float* a, int n, const MaskStages& st, int invert, long long* ids, long long* count,
                              unsigned char* mask, unsigned* part_asc, unsigned* part_desc, unsigned char* kept, int* block_cnt,
                              int* block_off, hipStream_t stream) {
  const MaskSplit m = mask_select_split(n);
  const dim3 grid(m.blocks, m.split);
  if (st.any_asc && st.any_desc)
    mask_rank_kernel<true, true><<<grid, MS_BLOCK, 0, stream>>>(a, n, m.chunk_len, part_asc, part_desc);
  else if (st.any_asc)
    mask_rank_kernel<true, false><<<grid, MS_BLOCK, 0, stream>>>(a, n, m.chunk_len, part_asc, part_desc);
  else
    mask_rank_kernel<false, true><<<grid, MS_BLOCK, 0, stream>>>(a, n, m.chunk_len, part_asc, part_desc);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  mask_flag_kernel<<<m.blocks, MS_BLOCK, 0, stream>>>(part_asc, part_desc, n, m.split, st, invert, kept, mask, block_cnt);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  mask_scan_kernel<<<1, 1024, 0, stream>>>(block_cnt, m.blocks, block_off, count);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  mask_place_kernel<<<m.blocks, MS_BLOCK, 0, stream>>>(kept, n, block_off, count, ids);
  return hipGetLastError();
}

hipError_t launch_mask_select_vote(const float* a, int n, int heads, const MaskStages& st, int invert, long long* ids,
                                   long long* count, unsigned char* mask, unsigned* part_asc, unsigned* part_desc,
                                   unsigned char* vote, int* hist, int* off, int* tot, unsigned char* kept, int* block_cnt,
                                   int* block_off, hipStream_t stream) {
  const MaskSplit m = mask_select_split(n);
  const dim3 grid(m.blocks, m.split, heads);
  if (st.any_asc && st.any_desc)
    mask_rank_heads_kernel<true, true><<<grid, MS_BLOCK, 0, stream>>>(a, n, m.chunk_len, part_asc, part_desc);
  else if (st.any_asc)
    mask_rank_heads_kernel<true, false><<<grid, MS_BLOCK, 0, stream>>>(a, n, m.chunk_len, part_asc, part_desc);
  else
    mask_rank_heads_kernel<false, true><<<grid, MS_BLOCK, 0, stream>>>(a, n, m.chunk_len, part_asc, part_desc);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  mask_vote_kernel<<<m.blocks, MS_BLOCK, 0, stream>>>(part_asc, part_desc, n, m.split, heads, st, vote, hist);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  mask_vote_scan_kernel<<<st.n * (heads + 1), 1024, 0, stream>>>(hist, m.blocks, heads, off, tot);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  mask_vote_flag_kernel<<<m.blocks, MS_BLOCK, 0, stream>>>(vote, off, tot, n, heads, st, invert, kept, mask, block_cnt);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  mask_scan_kernel<<<1, 1024, 0, stream>>>(block_cnt, m.blocks, block_off, count);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  mask_place_kernel<<<m.blocks, MS_BLOCK, 0, stream>>>(kept, n, block_off, count, ids);
  return hipGetLastError();
}

hipError_t launch_gather_rows(const float* src, const long long* ids, float* dst, long long n_rows, long long n_src, int dim,
                              hipStream_t stream) {
  gather_rows_kernel<<<rows_grid(n_rows * (dim / 4)), ROWS_BLOCK, 0, stream>>>(src, ids, dst, n_rows, n_src, dim / 4);
  return hipGetLastError();
}

hipError_t launch_scatter_rows(const float* src, const long long* ids, float* dst, long long n_rows, long long n_dst, int dim,
                               hipStream_t stream) {
  hipError_t e = hipMemsetAsync(dst, 0, (size_t)n_dst * dim * sizeof(float), stream);
  if (e != hipSuccess) return e;
  scatter_rows_kernel<<<rows_grid(n_rows * (dim / 4)), ROWS_BLOCK, 0, stream>>>(src, ids, dst, n_rows, n_dst, dim / 4);
  return hipGetLastError();
}
