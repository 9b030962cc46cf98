// api_mask.hip -- the C ABI of MHIM-MIL's mask selection and of the row gather / scatter (include/rrt_hip.h; kernels:
// mask_select.hip).  Host only: argument checks, the workspace carve, launches.
#include "api_internal.h"

using namespace rrt_api;

namespace {
struct MaskWs {
  unsigned *part_asc, *part_desc;
  unsigned char* kept;
  int *block_cnt, *block_off;
  size_t bytes;
};
// sized by bounds that grow with n (the split itself does not: see mask_select_split), so a larger bag never asks for less
MaskWs carve_mask(int64_t n, char* base) {
  MaskWs w{};
  const size_t part = (size_t)(n * MASK_SPLIT_MAX < MASK_SELECT_MAX_N ? n * MASK_SPLIT_MAX : MASK_SELECT_MAX_N);
  const size_t blocks = (size_t)(n + 255) / 256;
  Arena a{base};
  w.part_asc = a.take<unsigned>(part);
  w.part_desc = a.take<unsigned>(part);
  w.kept = a.take<unsigned char>((size_t)n);
  w.block_cnt = a.take<int>(blocks);
  w.block_off = a.take<int>(blocks);
  w.bytes = a.bytes();
  return w;
}
int check_mask_n(int64_t n, int32_t n_stages) {
  if (n <= 0 || n_stages < 1 || n_stages > 3) return RRT_E_INVALID;
  if (n > MASK_SELECT_MAX_N) return unsupported("mask_select: n above 262144");
  return RRT_OK;
}
struct MaskVoteWs {
  unsigned *part_asc, *part_desc;
  unsigned char *vote, *kept;
  int *hist, *off, *tot, *block_cnt, *block_off;
  size_t bytes;
};
// the single-head carve's bounds, with the parts once per head: never less for a larger n or for more heads
MaskVoteWs carve_mask_vote(int64_t n, int32_t heads, int32_t n_stages, char* base) {
  MaskVoteWs w{};
  const size_t part = (size_t)heads * (size_t)(n * MASK_SPLIT_MAX < MASK_SELECT_MAX_N ? n * MASK_SPLIT_MAX : MASK_SELECT_MAX_N);
  const size_t blocks = (size_t)(n + 255) / 256, classes = (size_t)n_stages * MASK_VOTE_VALUES;
  Arena a{base};
  w.part_asc = a.take<unsigned>(part);
  w.part_desc = a.take<unsigned>(part);
  w.vote = a.take<unsigned char>((size_t)n_stages * (size_t)n);
  w.hist = a.take<int>(classes * blocks);
  w.off = a.take<int>(classes * blocks);
  w.tot = a.take<int>(classes);
  w.kept = a.take<unsigned char>((size_t)n);
  w.block_cnt = a.take<int>(blocks);
  w.block_off = a.take<int>(blocks);
  w.bytes = a.bytes();
  return w;
}
int check_mask_vote(int64_t n, int32_t heads, int32_t n_stages) {
  if (heads < 1) return RRT_E_INVALID;
  const int rc = check_mask_n(n, n_stages);
  if (rc) return rc;
  if (heads > MASK_VOTE_MAX_HEADS) return unsupported("mask_select_vote: heads above 16");
  return RRT_OK;
}
int check_rows(const float* src, const int64_t* ids, float* dst, int64_t n_rows, int64_t n_other, int32_t dim) {
  if (!src || !ids || !dst || n_rows <= 0 || n_other <= 0 || dim <= 0) return RRT_E_INVALID;
  if (((uintptr_t)src | (uintptr_t)dst) & 15) return RRT_E_INVALID;
  if (dim % 4) return unsupported("gather / scatter rows: dim must be a multiple of 4");
  if (n_rows > ((int64_t)1 << 40) / dim || n_other > ((int64_t)1 << 40) / dim) return unsupported("gather / scatter rows: above 2^40 elements");
  return RRT_OK;
}
}  // namespace

int rrt_mask_select_workspace_size(int64_t n, int32_t n_stages, size_t* bytes) {
  if (!bytes) return RRT_E_INVALID;
  const int rc = check_mask_n(n, n_stages);
  if (rc) return rc;
  *bytes = carve_mask(n, nullptr).bytes;
  return RRT_OK;
}

int rrt_mask_select_f32(const float* a, int64_t n, const rrt_mask_stage* stages, int32_t n_stages, int32_t invert, int64_t* ids,
                        int64_t* count, uint8_t* mask, void* workspace, size_t workspace_bytes, void* stream) {
  if (!a || !stages || !ids || !count || !workspace) return RRT_E_INVALID;
  const int rc = check_mask_n(n, n_stages);
  if (rc) return rc;
  MaskStages st{};
  st.n = n_stages;
  for (int s = 0; s < n_stages; ++s) {
    if (stages[s].k < 1 || stages[s].k > n) return RRT_E_INVALID;
    st.largest[s] = stages[s].largest != 0;
    st.k[s] = (int)stages[s].k;
    st.pick[s] = stages[s].pick;
    (st.largest[s] ? st.any_desc : st.any_asc) = 1;
  }
  const MaskWs w = carve_mask(n, (char*)workspace);
  if (workspace_bytes < w.bytes) return RRT_E_WORKSPACE;
  RRT_TRY(launch_mask_select(a, (int)n, st, invert != 0, (long long*)ids, (long long*)count, mask, w.part_asc, w.part_desc, w.kept,
                             w.block_cnt, w.block_off, (hipStream_t)stream));
  return RRT_OK;
}

int rrt_mask_select_vote_workspace_size(int64_t n, int32_t heads, int32_t n_stages, size_t* bytes) {
  if (!bytes) return RRT_E_INVALID;
  const int rc = check_mask_vote(n, heads, n_stages);
  if (rc) return rc;
  *bytes = carve_mask_vote(n, heads, n_stages, nullptr).bytes;
  return RRT_OK;
}

int rrt_mask_select_vote_f32(const float* a, int64_t n, int32_t heads, const rrt_mask_stage* stages, int32_t n_stages, int32_t invert,
                             int64_t* ids, int64_t* count, uint8_t* mask, void* workspace, size_t workspace_bytes, void* stream) {
  if (!a || !stages || !ids || !count || !workspace) return RRT_E_INVALID;
  const int rc = check_mask_vote(n, heads, n_stages);
  if (rc) return rc;
  MaskStages st{};
  st.n = n_stages;
  for (int s = 0; s < n_stages; ++s) {
    if (stages[s].k < 1 || stages[s].k > n) return RRT_E_INVALID;
    st.largest[s] = stages[s].largest != 0;
    st.k[s] = (int)stages[s].k;
    st.pick[s] = stages[s].pick;
    (st.largest[s] ? st.any_desc : st.any_asc) = 1;
  }
  const MaskVoteWs w = carve_mask_vote(n, heads, n_stages, (char*)workspace);
  if (workspace_bytes < w.bytes) return RRT_E_WORKSPACE;
  RRT_TRY(launch_mask_select_vote(a, (int)n, heads, st, invert != 0, (long long*)ids, (long long*)count, mask, w.part_asc,
                                  w.part_desc, w.vote, w.hist, w.off, w.tot, w.kept, w.block_cnt, w.block_off,
                                  (hipStream_t)stream));
  return RRT_OK;
}

int rrt_gather_rows_f32(const float* src, const int64_t* ids, float* dst, int64_t n_rows, int64_t n_src, int32_t dim, void* stream) {
  const int rc = check_rows(src, ids, dst, n_rows, n_src, dim);
  if (rc) return rc;
  RRT_TRY(launch_gather_rows(src, (const long long*)ids, dst, n_rows, n_src, dim, (hipStream_t)stream));
  return RRT_OK;
}

int rrt_scatter_rows_f32(const float* src, const int64_t* ids, float* dst, int64_t n_rows, int64_t n_dst, int32_t dim, void* stream) {
  const int rc = check_rows(src, ids, dst, n_rows, n_dst, dim);
  if (rc) return rc;
  RRT_TRY(launch_scatter_rows(src, (const long long*)ids, dst, n_rows, n_dst, dim, (hipStream_t)stream));
  return RRT_OK;
}
