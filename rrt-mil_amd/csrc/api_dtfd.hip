// api_dtfd.hip -- the C ABI of DTFD-MIL (include/rrt_hip.h; kernels: segment_pool.hip): the score / segmented pool / backward
// stage entries and DTFD.test_forward as one call, built from the heads' shared front and the ABMIL tail of api.hip.  Host
// only: argument checks, the workspace carve, launches.
#include "api_internal.h"

using namespace rrt_api;

namespace {
constexpr int SEG_MAX_GROUPS = 64;

// (m_g, l_g) first: rrt_segment_pool_backward_f32 reads them from the workspace's first 2 * G floats
struct SegWs {
  float *ml, *part, *z;
  size_t bytes;
};
SegWs carve_seg(int64_t N, int dim, int C, int G, char* base) {
  SegWs w{};
  Arena a{base};
  w.ml = a.take(2 * (size_t)G);
  w.part = a.take(segment_pool_parts((int)N, G) * ((size_t)dim + 4));
  w.z = a.take((size_t)N * C);
  w.bytes = a.bytes();
  return w;
}
int check_seg(int64_t N, int dim, int C, int G) {
  if (N <= 0 || dim <= 0 || C <= 0 || G <= 0) return RRT_E_INVALID;
  if (dim % 32) return unsupported("segment pool: dim must be a multiple of 32");
  if (dim > 2048) return unsupported("segment pool: dim > 2048");
  if (C > 8) return unsupported("segment pool: 1 <= n_classes <= 8");
  if (G > SEG_MAX_GROUPS) return unsupported("segment pool: 1 <= n_groups <= 64");
  if (N < G)
    return unsupported("segment pool: n_tokens < n_groups (the reference lets the empty chunks add no rows; this library refuses the bag)");
  if (N > (int64_t)1000000) return unsupported("segment pool: bag larger than 1e6 tokens");
  return RRT_OK;
}
int check_scores(int64_t N, int hidden) {
  if (N <= 0 || hidden <= 0) return RRT_E_INVALID;
  if (hidden % 4) return unsupported("gate scores: hidden width must be a multiple of 4");
  if (N > (int64_t)1000000) return unsupported("gate scores: bag larger than 1e6 tokens");
  return RRT_OK;
}
bool misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

HeadFront head_front(const rrt_dtfd_desc* d) { return HeadFront{&d->enc, d->input_dim, d->emb_act, d->has_rrt, 0}; }
int dtfd_rows(const rrt_dtfd_desc* d) { return d->distill == RRT_DTFD_MAXMINS ? 2 * d->group : d->group; }

int check_dtfd(const rrt_dtfd_desc* d, int64_t N) {
  if (!d) return RRT_E_INVALID;
  int rc = check_head_front(head_front(d), N);
  if (rc) return rc;
  if (d->distill < RRT_DTFD_MAXMINS || d->distill > RRT_DTFD_AFS) return unsupported("dtfd: distill must be RRT_DTFD_*");
  rc = check_scores(N, d->hidden);
  if (rc) return rc;
  rc = check_seg(N, d->enc.dim, d->n_classes, d->group);
  if (rc) return rc;
  return check_pool(dtfd_rows(d), d->enc.dim, d->hidden, RRT_ACT_TANH, d->n_classes);
}

// the head's scratch behind the shared front: tier 1's gate rows, scores and segmented pool, the distilled rows, tier 2's pool
struct DtfdWs {
  float *hid_a, *hid_b, *a, *pooled, *rows;
  long long *sel, *ids;
  SegWs seg;
  PoolWs pool;
  size_t bytes;
};
DtfdWs carve_dtfd_scratch(const rrt_dtfd_desc* d, int64_t N, char* base) {
  DtfdWs w{};
  Arena a{base};
  const int D = d->enc.dim, R = dtfd_rows(d);
  w.hid_a = a.take((size_t)N * d->hidden);
  w.hid_b = a.take((size_t)N * d->hidden);
  w.a = a.take((size_t)N);
  w.pooled = a.take((size_t)d->group * D);
  w.rows = a.take((size_t)R * D);
  w.sel = a.take<long long>(2 * (size_t)d->group);
  w.ids = a.take<long long>(2 * (size_t)d->group);
  w.seg = carve_seg(N, D, d->n_classes, d->group, a.take<char>(carve_seg(N, D, d->n_classes, d->group, nullptr).bytes));
  w.pool = carve_pool(R, D, d->hidden, 1, a.take<char>(carve_pool(R, D, d->hidden, 1, nullptr).bytes));
  w.bytes = a.bytes();
  return w;
}
int carve_dtfd(const rrt_dtfd_desc* d, int64_t N, char* base, HeadWs* hw, DtfdWs* dws) {
  int rc = carve_head(head_front(d), N, carve_dtfd_scratch(d, N, nullptr).bytes, d->hidden, base, hw);
  if (rc == RRT_OK && dws) *dws = carve_dtfd_scratch(d, N, hw->head);
  return rc;
}
}  // namespace

int rrt_segment_pool_workspace_size(int64_t n_tokens, int32_t dim, int32_t n_classes, int32_t n_groups, size_t* bytes) {
  if (!bytes) return RRT_E_INVALID;
  const int rc = check_seg(n_tokens, dim, n_classes, n_groups);
  if (rc) return rc;
  *bytes = carve_seg(n_tokens, dim, n_classes, n_groups, nullptr).bytes;
  return RRT_OK;
}

int rrt_gate_scores_f32(const float* hid_a, const float* hid_b, const float* c_w, const float* c_b, float* a, int64_t n_tokens,
                        int32_t hidden, void* stream) {
  if (!hid_a || !c_w || !a) return RRT_E_INVALID;
  const int rc = check_scores(n_tokens, hidden);
  if (rc) return rc;
  if (misaligned(hid_a) || misaligned(hid_b) || misaligned(c_w)) return RRT_E_INVALID;
  RRT_TRY(launch_gate_scores(hid_a, hid_b, c_w, c_b, a, (int)n_tokens, hidden, (hipStream_t)stream));
  return RRT_OK;
}

int rrt_segment_pool_f32(const float* mid, const float* a, const int64_t* perm, const float* cls_w, float* pooled, int64_t* sel,
                         float* attn, float* p, int64_t n_tokens, int32_t dim, int32_t n_classes, int32_t n_groups,
                         void* workspace, size_t workspace_bytes, void* stream) {
  if (!mid || !a || !cls_w || !pooled || !sel) return RRT_E_INVALID;
  const int rc = check_seg(n_tokens, dim, n_classes, n_groups);
  if (rc) return rc;
  if (misaligned(mid) || misaligned(cls_w) || misaligned(pooled)) return RRT_E_INVALID;
  const SegWs w = carve_seg(n_tokens, dim, n_classes, n_groups, (char*)workspace);
  if (!workspace || workspace_bytes < w.bytes) return RRT_E_WORKSPACE;
  RRT_TRY(launch_segment_pool(mid, a, (const long long*)perm, cls_w, pooled, (long long*)sel, attn, p, w.ml, w.part, w.z, nullptr,
                              0, (int)n_tokens, dim, n_classes, n_groups, (hipStream_t)stream));
  return RRT_OK;
}

int rrt_segment_pool_backward_f32(const float* mid, const float* a, const int64_t* perm, const float* pooled,
                                  const float* d_pooled, float* d_mid, float* d_a, int64_t n_tokens, int32_t dim,
                                  int32_t n_groups, void* workspace, size_t workspace_bytes, void* stream) {
  if (!mid || !a || !pooled || !d_pooled || !d_mid || !d_a) return RRT_E_INVALID;
  const int rc = check_seg(n_tokens, dim, 1, n_groups);
  if (rc) return rc;
  if (misaligned(mid) || misaligned(d_mid)) return RRT_E_INVALID;
  // the forward's workspace, whatever its n_classes was: (m_g, l_g) are its first piece
  if (!workspace || workspace_bytes < carve_seg(n_tokens, dim, 1, n_groups, nullptr).bytes) return RRT_E_WORKSPACE;
  RRT_TRY(launch_segment_pool_backward(mid, a, (const long long*)perm, pooled, d_pooled, (const float*)workspace, d_mid, d_a,
                                       (int)n_tokens, dim, n_groups, (hipStream_t)stream));
  return RRT_OK;
}

int rrt_dtfd_workspace_size(const rrt_dtfd_desc* desc, int64_t n_tokens, size_t* bytes) {
  if (!bytes) return RRT_E_INVALID;
  int rc = check_dtfd(desc, n_tokens);
  if (rc) return rc;
  HeadWs hw;
  rc = carve_dtfd(desc, n_tokens, nullptr, &hw, nullptr);
  if (rc) return rc;
  *bytes = hw.bytes;
  return RRT_OK;
}

int rrt_dtfd_forward_f32(const rrt_dtfd_desc* desc, const rrt_dtfd_weights* w, const float* x, const int64_t* perm, float* logits,
                         int64_t* sel, float* p, int64_t n_tokens, void* workspace, size_t workspace_bytes, void* stream) {
  if (!desc || !w || !x || !logits) return RRT_E_INVALID;
  int rc = check_dtfd(desc, n_tokens);
  if (rc) return rc;
  if (!w->emb_w || !w->att_v_w || !w->att_u_w || !w->att_w_w || !w->cls_w || !w->u_v_w || !w->u_u_w || !w->u_w_w || !w->u_fc_w)
    return RRT_E_INVALID;
  HeadWs hw;
  DtfdWs dws;
  rc = carve_dtfd(desc, n_tokens, (char*)workspace, &hw, &dws);
  if (rc) return rc;
  if (!workspace || workspace_bytes < hw.bytes) return RRT_E_WORKSPACE;
  const int N = (int)n_tokens, D = desc->enc.dim, H = desc->hidden, C = desc->n_classes, G = desc->group, R = dtfd_rows(desc);
  const int prec = gemm_precision(desc->enc.compute);
  hipStream_t st = (hipStream_t)stream;
  bool p16 = false;
  rc = head_front_forward(head_front(desc), hw, x, w->emb_w, nullptr, &w->enc, w->att_v_w, w->att_u_w, H, nullptr, /*tuning=*/false,
                          n_tokens, stream, &p16);
  if (rc) return rc;
  // tier 1's gate, as pool_predict runs it; the scores, the pool, the CAM and the selection are fp32 in every mode
  p16 = p16 && D % 64 == 0 && (prec == RRT_COMPUTE_BF16 || prec == RRT_COMPUTE_F16);
  LinearEpilogue ep{};
  ep.prec = prec;
  ep.bias = w->att_v_b;
  ep.act = RRT_ACT_TANH;
  RRT_TRY(p16 ? launch_linear16(hw.y16, hw.pa16, dws.hid_a, N, H, D, ep, st) : launch_linear(hw.y, w->att_v_w, dws.hid_a, N, H, D, ep, st));
  ep.bias = w->att_u_b;
  ep.act = RRT_ACT_SIGMOID;
  RRT_TRY(p16 ? launch_linear16(hw.y16, hw.pb16, dws.hid_b, N, H, D, ep, st) : launch_linear(hw.y, w->att_u_w, dws.hid_b, N, H, D, ep, st));
  RRT_TRY(launch_gate_scores(dws.hid_a, dws.hid_b, w->att_w_w, w->att_w_b, dws.a, N, H, st));
  const bool afs = desc->distill == RRT_DTFD_AFS;
  RRT_TRY(launch_segment_pool(hw.y, dws.a, (const long long*)perm, w->cls_w, dws.pooled, sel ? (long long*)sel : dws.sel, nullptr, p,
                              dws.seg.ml, dws.seg.part, dws.seg.z, afs ? nullptr : dws.ids,
                              desc->distill == RRT_DTFD_MAXMINS ? 2 : 1, N, D, C, G, st));
  const float* rows = dws.pooled;
  if (!afs) {
    RRT_TRY(launch_gather_rows(hw.y, dws.ids, dws.rows, R, n_tokens, D, st));
    rows = dws.rows;
  }
  return pool_predict(rows, w->u_v_w, w->u_v_b, w->u_u_w, w->u_u_b, w->u_w_w, w->u_w_b, w->u_fc_w, w->u_fc_b, nullptr, logits,
                      nullptr, 0, R, D, H, RRT_ACT_TANH, C, prec, dws.pool, st);
}
