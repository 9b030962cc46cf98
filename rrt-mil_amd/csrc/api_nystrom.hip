// api_nystrom.hip -- Nystrom attention and the TransMIL baseline composed on its carved structs (include/rrt_hip.h: Nystrom
// forward, stages, attention rows and backward; TransMIL forward, attention maps and the one-call training step).
#include <math.h>

#include "api_internal.h"

using namespace rrt_api;

namespace {
// ---- Nystrom attention (nystrom.hip)
int check_nystrom_heads(int32_t heads) {
  if (heads < 1 || heads > 16) return unsupported("nystrom: heads must be in 1..16");
  return RRT_OK;
}
int check_nystrom_np(int64_t np) {
  if (np <= 0) return RRT_E_INVALID;
  if (np % 256) return unsupported("nystrom: n_padded must be a multiple of num_landmarks = 256");
  if (np > 1000000 + 255) return unsupported("nystrom: n above 1e6");
  return RRT_OK;
}
int check_nystrom(const rrt_nystrom_desc* d, int64_t n) {
  if (!d || n <= 0) return RRT_E_INVALID;
  if (d->dim_head != 64) return unsupported("nystrom: dim_head must be 64");
  if (d->num_landmarks != 256) return unsupported("nystrom: num_landmarks must be 256");
  if (d->residual && (d->residual_conv_kernel < 1 || d->residual_conv_kernel % 2 == 0 || d->residual_conv_kernel > 63))
    return unsupported("nystrom: residual_conv_kernel must be odd and <= 63");
  if (d->pinv_iterations < 1 || d->pinv_iterations > 16) return unsupported("nystrom: pinv_iterations must be in 1..16");
  int rc = check_nystrom_heads(d->heads);
  if (rc) return rc;
  if (d->dim <= 0 || d->dim % 32 || d->dim > 1024) return unsupported("nystrom: dim must be a multiple of 32, at most 1024");
  if (n > 1000000) return unsupported("nystrom: n above 1e6");
  return RRT_OK;
}

int check_nystrom_batch(int64_t b) {
  if (b < 1 || b > 4096) return unsupported("nystrom: batch b must be in 1..4096");
  return RRT_OK;
}

struct NystromWs {
  float *qkv, *ql, *kl, *a2, *z, *av, *wz, *o, *lattn, *pinv;
  float *qkv_c, *o_c;      // b > 1 with front padding: the two linears' compact [b * n] rows (nystrom_batched_front)
  int64_t np, b;
  size_t bytes;
};
// with_o = false: without o (the one-call TransMIL step's layer 2 needs one row of it, kept elsewhere)
// b sequences: every piece b times as large, in the same order (b = 1 is the single-sequence layout)
NystromWs carve_nystrom(const rrt_nystrom_desc* d, int64_t n, char* base, bool with_o = true, int64_t b = 1) {
  NystromWs ws{};
  const int64_t np = (n + 255) / 256 * 256;
  const size_t hd = (size_t)d->heads * 64, lm = (size_t)b * d->heads * 256 * 64, mm = (size_t)b * d->heads * 256 * 256;
  Arena a{base};
  ws.np = np;
  ws.b = b;
  ws.qkv = a.take((size_t)b * np * 3 * hd);
  ws.ql = a.take(lm);
  ws.kl = a.take(lm);
  ws.a2 = a.take(mm);
  ws.z = a.take(mm);
  ws.av = a.take(lm);
  ws.wz = a.take(lm);
  if (with_o) ws.o = a.take((size_t)b * np * hd);
  ws.lattn = a.take(nystrom_lattn_floats((long)np, d->heads, (int)b));
  ws.pinv = a.take(nystrom_pinv_floats(d->heads, (int)b));
  if (b > 1 && np != n) {
    ws.qkv_c = a.take((size_t)b * n * 3 * hd);
    ws.o_c = a.take((size_t)b * n * hd);
  }
  ws.bytes = a.bytes();
  return ws;
}

// the stages in front of the output: to_qkv, the landmarks, both landmark softmaxes, the pseudo-inverse and wz = z av
int nystrom_front(const rrt_nystrom_desc* d, const rrt_nystrom_weights* w, const float* x, int64_t n, const NystromWs& ws,
                  hipStream_t st, float* lse) {
  const int hd = d->heads * 64;
  const int64_t pad = ws.np - n;
  if (pad) RRT_TRY(hipMemsetAsync(ws.qkv, 0, (size_t)pad * 3 * hd * sizeof(float), st));
  LinearEpilogue ep{};
  ep.q_cols = hd;
  ep.q_scale = 0.125f;                       // dim_head^-0.5, dim_head = 64
  RRT_TRY(launch_linear(x, w->qkv_w, ws.qkv + (size_t)pad * 3 * hd, (int)n, 3 * hd, d->dim, ep, st));
  RRT_TRY(launch_nystrom_landmarks(ws.qkv, ws.ql, ws.kl, (long)ws.np, d->heads, st));
  RRT_TRY(launch_nystrom_sim2(ws.ql, ws.kl, ws.a2, d->heads, st));
  RRT_TRY(launch_nystrom_lattn(ws.qkv, ws.ql, ws.av, ws.lattn, (long)ws.np, d->heads, st, lse));
  RRT_TRY(launch_nystrom_pinv(ws.a2, ws.z, ws.pinv, d->heads, d->pinv_iterations, st));
  RRT_TRY(launch_nystrom_zav(ws.z, ws.av, ws.wz, d->heads, st));
  return RRT_OK;
}

// y [n, dim] = NystromAttention(x); everything checked by the caller
int nystrom_forward(const rrt_nystrom_desc* d, const rrt_nystrom_weights* w, const float* x, float* y, int64_t n,
                    const NystromWs& ws, hipStream_t st, float* lse = nullptr) {
  const int hd = d->heads * 64;
  const int64_t pad = ws.np - n;
  const int rc = nystrom_front(d, w, x, n, ws, st, lse);
  if (rc) return rc;
  RRT_TRY(launch_nystrom_output(ws.qkv, ws.kl, ws.wz, d->residual ? w->conv_w : nullptr, ws.o, (long)ws.np, d->heads,
                                d->residual_conv_kernel, st));
  LinearEpilogue eo{};
  eo.bias = w->out_b;
  RRT_TRY(launch_linear(ws.o + (size_t)pad * hd, w->out_w, y, (int)n, d->dim, hd, eo, st));
  return RRT_OK;
}

bool nystrom_weights_ok(const rrt_nystrom_desc* d, const rrt_nystrom_weights* w) {
  return w->qkv_w && w->out_w && w->out_b && (!d->residual || w->conv_w);
}

// ---- b > 1 sequences of n tokens, x [b * n, dim] -> the attention output in front of to_out, o [b * n, heads * 64] COMPACT (the
// returned pointer: ws.o itself when n is a multiple of 256).  One launch per stage.  The front-padded layout: to_qkv runs on the
// b * n real rows alone (the pad rows are zero whatever the weights: no bias), and two strided copies move its rows behind each
// item's zeroed pad rows and the output's real rows back -- a quarter more traffic than the attention's own, against up to
// np / n times the flops of both linears on zero rows.
int nystrom_batched_front(const rrt_nystrom_desc* d, const rrt_nystrom_weights* w, const float* x, int64_t n, const NystromWs& ws,
                          hipStream_t st, const float** o_compact, float* lse = nullptr) {
  const int hd = d->heads * 64, b = (int)ws.b;
  const int64_t pad = ws.np - n;
  const size_t row3 = (size_t)3 * hd * sizeof(float), row1 = (size_t)hd * sizeof(float);
  LinearEpilogue ep{};
  ep.q_cols = hd;
  ep.q_scale = 0.125f;                       // dim_head^-0.5, dim_head = 64
  RRT_TRY(launch_linear(x, w->qkv_w, pad ? ws.qkv_c : ws.qkv, (int)(b * n), 3 * hd, d->dim, ep, st));
  if (pad) {
    RRT_TRY(hipMemset2DAsync(ws.qkv, (size_t)ws.np * row3, 0, (size_t)pad * row3, (size_t)b, st));
    RRT_TRY(hipMemcpy2DAsync(ws.qkv + (size_t)pad * 3 * hd, (size_t)ws.np * row3, ws.qkv_c, (size_t)n * row3, (size_t)n * row3,
                             (size_t)b, hipMemcpyDeviceToDevice, st));
  }
  RRT_TRY(launch_nystrom_landmarks(ws.qkv, ws.ql, ws.kl, (long)ws.np, d->heads, st, b));
  RRT_TRY(launch_nystrom_sim2(ws.ql, ws.kl, ws.a2, d->heads, st, b));
  RRT_TRY(launch_nystrom_lattn(ws.qkv, ws.ql, ws.av, ws.lattn, (long)ws.np, d->heads, st, lse, b));
  RRT_TRY(launch_nystrom_pinv(ws.a2, ws.z, ws.pinv, d->heads, d->pinv_iterations, st, b));
  RRT_TRY(launch_nystrom_zav(ws.z, ws.av, ws.wz, d->heads, st, b));
  RRT_TRY(launch_nystrom_output(ws.qkv, ws.kl, ws.wz, d->residual ? w->conv_w : nullptr, ws.o, (long)ws.np, d->heads,
                                d->residual_conv_kernel, st, b));
  if (pad)
    RRT_TRY(hipMemcpy2DAsync(ws.o_c, (size_t)n * row1, ws.o + (size_t)pad * hd, (size_t)ws.np * row1, (size_t)n * row1, (size_t)b,
                             hipMemcpyDeviceToDevice, st));
  *o_compact = pad ? ws.o_c : ws.o;
  return RRT_OK;
}

// the product b * n of a batched call stays within what one linear takes
int check_nystrom_rows(int64_t b, int64_t n) {
  if (b * n > 4000000) return unsupported("nystrom: b * n above 4e6");
  return RRT_OK;
}

// what a query row of the attention matrix needs on top of a forward's workspace of `front` bytes: lse | r, [heads, 256] each
struct RowWs {
  float *lse, *r;
  size_t bytes;
};
RowWs carve_row(size_t front, int heads, char* base) {
  RowWs ws{};
  Arena a{base};
  a.take<char>(front);
  ws.lse = a.take((size_t)heads * 256);
  ws.r = a.take((size_t)heads * 256);
  ws.bytes = a.bytes();
  return ws;
}

// row `row` (of the n unpadded rows) of the approximated attention matrix, columns 0 .. n - 1 -> attn [heads, n]; ws is as
// nystrom_forward left it, with rw.lse filled by the same forward
int nystrom_row(const rrt_nystrom_desc* d, int64_t row, float* attn, int64_t n, const NystromWs& ws, const RowWs& rw,
                hipStream_t st) {
  const int64_t pad = ws.np - n;
  RRT_TRY(launch_nystrom_attn_row(ws.qkv, ws.ql, ws.kl, ws.z, rw.lse, rw.r, attn, (long)(pad + row), (long)ws.np, (long)pad,
                                  (long)n, d->heads, st));
  return RRT_OK;
}

// ---- Nystrom attention: training (nystrom_bwd.hip)
// the forward's workspace kept whole (what the backward reads: qkv, ql, kl, a2, z, av, wz, o) | lse [b, heads, 256]
struct NystromStash {
  NystromWs f;
  float* lse;
  size_t bytes;
};
NystromStash carve_nystrom_stash(const rrt_nystrom_desc* d, int64_t n, char* base, bool with_o = true, int64_t b = 1) {
  NystromStash s{};
  s.f = carve_nystrom(d, n, base, with_o, b);
  Arena a{base};
  a.take<char>(s.f.bytes);
  s.lse = a.take((size_t)b * d->heads * 256);
  s.bytes = a.bytes();
  return s;
}

size_t max_sz(size_t a, size_t b) { return a > b ? a : b; }

struct NystromBwdWs {
  float *d_o, *d_qkv, *d_ql, *d_kl, *d_wz, *d_av, *d_z, *part, *pinv;
  char* lin;
  float *d_o_c, *d_qkv_c;  // b > 1 with front padding: the two linears' compact [b * n] rows, as the forward's qkv_c / o_c
  size_t bytes;
};
// b sequences: every piece b times as large, in the same order (b = 1 is the single-sequence layout)
NystromBwdWs carve_nystrom_bwd(const rrt_nystrom_desc* d, int64_t n, char* base, int64_t b = 1) {
  NystromBwdWs ws{};
  const int64_t np = (n + 255) / 256 * 256;
  const int hd = d->heads * 64, ib = (int)b;
  const size_t lm = (size_t)b * d->heads * 256 * 64, mm = (size_t)b * d->heads * 256 * 256;
  Arena a{base};
  ws.d_o = a.take((size_t)b * np * hd);
  ws.d_qkv = a.take((size_t)b * np * 3 * hd);
  ws.d_ql = a.take(lm);
  ws.d_kl = a.take(lm);
  ws.d_wz = a.take(lm);
  ws.d_av = a.take(lm);
  ws.d_z = a.take(mm);
  ws.part = a.take(max_sz(nystrom_output_bwd_floats((long)np, d->heads, ib), nystrom_lattn_bwd_floats((long)np, d->heads, ib)));
  ws.pinv = a.take(nystrom_pinv_bwd_floats(d->heads, d->pinv_iterations, ib));
  ws.lin = a.take<char>(max_sz(linear_bwd_workspace((int)(b * n), d->dim, hd), linear_bwd_workspace((int)(b * n), 3 * hd, d->dim)));
  if (b > 1 && np != n) {
    ws.d_o_c = a.take((size_t)b * n * hd);
    ws.d_qkv_c = a.take((size_t)b * n * 3 * hd);
  }
  ws.bytes = a.bytes();
  return ws;
}

struct LattnBwdWs {
  float *fwd, *av, *lse, *bwd;
  size_t bytes;
};
LattnBwdWs carve_lattn_bwd(int64_t np, int heads, char* base, int b = 1) {
  LattnBwdWs ws{};
  Arena a{base};
  ws.fwd = a.take(nystrom_lattn_floats((long)np, heads, b));
  ws.av = a.take((size_t)b * heads * 256 * 64);
  ws.lse = a.take((size_t)b * heads * 256);
  ws.bwd = a.take(nystrom_lattn_bwd_floats((long)np, heads, b));
  ws.bytes = a.bytes();
  return ws;
}

struct PinvSimBwdWs {
  float *a2, *bwd;
  size_t bytes;
};
PinvSimBwdWs carve_pinv_sim_bwd(int heads, int iters, char* base, int b = 1) {
  PinvSimBwdWs ws{};
  Arena a{base};
  ws.a2 = a.take((size_t)b * heads * 256 * 256);
  ws.bwd = a.take(nystrom_pinv_bwd_floats(heads, iters, b));
  ws.bytes = a.bytes();
  return ws;
}

int check_pinv_iterations(int32_t iterations) {
  if (iterations < 1 || iterations > 16) return unsupported("nystrom: pinv_iterations must be in 1..16");
  return RRT_OK;
}
int check_np_heads(int64_t np, int32_t heads) {
  int rc = check_nystrom_np(np);
  if (!rc) rc = check_nystrom_heads(heads);
  return rc;
}

// the backward behind d_qkv (q and v thirds written, k third zeroed), d_kl and d_wz, which the output stage's adjoint left in
// b: wz = z av, both landmark softmaxes, the pseudo-inverse, the landmarks and to_qkv.  Writes grads->qkv_w and, unless NULL, dx.
int nystrom_backward_rest(const rrt_nystrom_desc* desc, const rrt_nystrom_weights* w, const float* x, const NystromStash& s,
                          const NystromBwdWs& b, const rrt_nystrom_grads* grads, float* dx, int64_t n, hipStream_t st) {
  const int heads = desc->heads, hd = heads * 64;
  const long np = (long)s.f.np;
  const int64_t pad = s.f.np - n;
  RRT_TRY(launch_nystrom_zav_backward(s.f.z, s.f.av, b.d_wz, b.d_z, b.d_av, heads, st));
  RRT_TRY(launch_nystrom_lattn_backward(s.f.qkv, s.f.ql, s.f.av, s.lse, b.d_av, b.d_qkv, b.d_ql, b.part, np, heads, st));
  RRT_TRY(launch_nystrom_pinv_sim_backward(s.f.ql, s.f.kl, s.f.a2, b.d_z, b.d_ql, b.d_kl, 1, b.pinv, heads,
                                           desc->pinv_iterations, st));
  RRT_TRY(launch_nystrom_landmarks_backward(b.d_ql, b.d_kl, b.d_qkv, np, heads, st));
  // to_qkv: the forward scales q in the linear's epilogue; the pad rows of dx are dropped
  float* d_rows = b.d_qkv + (size_t)pad * 3 * hd;
  RRT_TRY(launch_nystrom_scale_q(d_rows, (long)n, heads, st));
  RRT_TRY(launch_linear_backward(d_rows, x, w->qkv_w, dx, grads->qkv_w, nullptr, (int)n, 3 * hd, desc->dim, RRT_COMPUTE_F32,
                                 b.lin, st));
  return RRT_OK;
}

// rrt_nystrom_attention_backward_f32 on carved structs; everything checked by the caller
int nystrom_backward(const rrt_nystrom_desc* desc, const rrt_nystrom_weights* w, const float* x, const float* dy,
                     const NystromStash& s, const NystromBwdWs& b, const rrt_nystrom_grads* grads, float* dx, int64_t n,
                     hipStream_t st) {
  const int heads = desc->heads, hd = heads * 64;
  const long np = (long)s.f.np;
  const int64_t pad = s.f.np - n;
  // to_out: the pad rows of d_o are zero
  if (pad) RRT_TRY(hipMemsetAsync(b.d_o, 0, (size_t)pad * hd * sizeof(float), st));
  RRT_TRY(launch_linear_backward(dy, s.f.o + (size_t)pad * hd, w->out_w, b.d_o + (size_t)pad * hd, grads->out_w, grads->out_b,
                                 (int)n, desc->dim, hd, RRT_COMPUTE_F32, b.lin, st));
  RRT_TRY(launch_nystrom_output_backward(s.f.qkv, s.f.kl, s.f.wz, desc->residual ? w->conv_w : nullptr, b.d_o, b.d_qkv, b.d_kl,
                                         b.d_wz, grads->conv_w, b.part, np, heads, desc->residual_conv_kernel, st));
  return nystrom_backward_rest(desc, w, x, s, b, grads, dx, n, st);
}

// ---- b > 1 sequences, training.  The item rides in blockIdx.z of the tile kernels and in the batch (z) of the backward's
// matrix products, b * heads of them: 2048 * 16 stays within a grid's 65535.
int check_nystrom_train_batch(int64_t b) {
  if (b < 1 || b > 2048) return unsupported("nystrom: training batch b must be in 1..2048");
  return RRT_OK;
}

// rrt_nystrom_attention_batched_backward_f32 on carved structs, b > 1; everything checked by the caller.  The adjoint of
// nystrom_batched_front: both linears run on the b * n real rows, d_o's pad rows (in FRONT of each item) are zero, d_qkv's are
// dropped; n a multiple of 256 works in place.
int nystrom_backward_batched(const rrt_nystrom_desc* desc, const rrt_nystrom_weights* w, const float* x, const float* dy,
                             const NystromStash& s, const NystromBwdWs& bw, const rrt_nystrom_grads* grads, float* dx, int64_t n,
                             hipStream_t st) {
  const int heads = desc->heads, hd = heads * 64, b = (int)s.f.b;
  const long np = (long)s.f.np;
  const int64_t pad = s.f.np - n, rows = (int64_t)b * n;
  const size_t row3 = (size_t)3 * hd * sizeof(float), row1 = (size_t)hd * sizeof(float);
  RRT_TRY(launch_linear_backward(dy, pad ? s.f.o_c : s.f.o, w->out_w, pad ? bw.d_o_c : bw.d_o, grads->out_w, grads->out_b,
                                 (int)rows, desc->dim, hd, RRT_COMPUTE_F32, bw.lin, st));
  if (pad) {
    RRT_TRY(hipMemset2DAsync(bw.d_o, (size_t)np * row1, 0, (size_t)pad * row1, (size_t)b, st));
    RRT_TRY(hipMemcpy2DAsync(bw.d_o + (size_t)pad * hd, (size_t)np * row1, bw.d_o_c, (size_t)n * row1, (size_t)n * row1, (size_t)b,
                             hipMemcpyDeviceToDevice, st));
  }
  RRT_TRY(launch_nystrom_output_backward(s.f.qkv, s.f.kl, s.f.wz, desc->residual ? w->conv_w : nullptr, bw.d_o, bw.d_qkv, bw.d_kl,
                                         bw.d_wz, grads->conv_w, bw.part, np, heads, desc->residual_conv_kernel, st, b));
  RRT_TRY(launch_nystrom_zav_backward(s.f.z, s.f.av, bw.d_wz, bw.d_z, bw.d_av, heads, st, b));
  RRT_TRY(launch_nystrom_lattn_backward(s.f.qkv, s.f.ql, s.f.av, s.lse, bw.d_av, bw.d_qkv, bw.d_ql, bw.part, np, heads, st, b));
  RRT_TRY(launch_nystrom_pinv_sim_backward(s.f.ql, s.f.kl, s.f.a2, bw.d_z, bw.d_ql, bw.d_kl, 1, bw.pinv, heads,
                                           desc->pinv_iterations, st, b));
  RRT_TRY(launch_nystrom_landmarks_backward(bw.d_ql, bw.d_kl, bw.d_qkv, np, heads, st, b));
  float* d_rows = bw.d_qkv;
  if (pad) {
    RRT_TRY(hipMemcpy2DAsync(bw.d_qkv_c, (size_t)n * row3, bw.d_qkv + (size_t)pad * 3 * hd, (size_t)np * row3, (size_t)n * row3,
                             (size_t)b, hipMemcpyDeviceToDevice, st));
    d_rows = bw.d_qkv_c;
  }
  RRT_TRY(launch_nystrom_scale_q(d_rows, (long)rows, heads, st));
  RRT_TRY(launch_linear_backward(d_rows, x, w->qkv_w, dx, grads->qkv_w, nullptr, (int)rows, 3 * hd, desc->dim, RRT_COMPUTE_F32,
                                 bw.lin, st));
  return RRT_OK;
}

int check_nystrom_train_batched(const rrt_nystrom_desc* desc, int64_t b, int64_t n) {
  int rc = check_nystrom(desc, n);
  if (!rc) rc = check_nystrom_train_batch(b);
  if (!rc) rc = check_nystrom_rows(b, n);
  return rc;
}
int check_stage_batched(int64_t b, int32_t heads) {
  int rc = check_nystrom_heads(heads);
  if (!rc) rc = check_nystrom_train_batch(b);
  return rc;
}
int check_stage_batched(int64_t b, int64_t np, int32_t heads) {
  int rc = check_np_heads(np, heads);
  if (!rc) rc = check_nystrom_train_batch(b);
  return rc;
}

int check_output_row(int64_t row, int64_t np, int32_t heads, const float* conv_w, int32_t conv_k) {
  int rc = check_np_heads(np, heads);
  if (rc) return rc;
  if (row < 0 || row >= np) return unsupported("nystrom: row must be in [0, n_padded)");
  if (conv_w && (conv_k < 1 || conv_k % 2 == 0 || conv_k > 63)) return unsupported("nystrom: residual_conv_kernel must be odd and <= 63");
  return RRT_OK;
}

// ---- the TransMIL baseline (nystrom.hip, peg.hip): fc1, the cls token and the square padding, two Nystrom layers around PPEG
int ceil_sqrt_i64(int64_t n) {
  int64_t h = (int64_t)ceil(sqrt((double)n));
  while (h * h < n) ++h;
  while (h > 1 && (h - 1) * (h - 1) >= n) --h;
  return (int)h;
}

int check_transmil(const rrt_transmil_desc* d, int64_t N) {
  if (!d || N <= 0) return RRT_E_INVALID;
  if (N > 998001) return unsupported("transmil: n_tokens above 998001 (the 1 + H * H rows must stay within nystrom's n <= 1e6)");
  int rc = check_nystrom(&d->attn, N);
  if (rc) return rc;
  if (d->input_dim <= 0 || d->input_dim % 32) return unsupported("input_dim must be a positive multiple of 32");
  if (d->act != RRT_ACT_NONE && d->act != RRT_ACT_RELU && d->act != RRT_ACT_GELU) return unsupported("transmil: act must be none/relu/gelu");
  if (d->n_classes < 1 || d->n_classes > 64) return unsupported("transmil: n_classes must be in 1..64");
  return RRT_OK;
}

struct TransmilWs {
  float *emb, *seq, *seq2, *ln, *att;
  char* nys;
  int64_t rows;
  int side;
  size_t bytes;
};
TransmilWs carve_transmil(const rrt_transmil_desc* d, int64_t N, char* base) {
  TransmilWs ws{};
  ws.side = ceil_sqrt_i64(N);
  ws.rows = 1 + (int64_t)ws.side * ws.side;
  const size_t D = (size_t)d->attn.dim;
  Arena a{base};
  ws.emb = a.take((size_t)N * D);
  ws.seq = a.take((size_t)ws.rows * D);
  ws.seq2 = a.take((size_t)ws.rows * D);
  ws.ln = a.take((size_t)ws.rows * D);
  ws.att = a.take((size_t)ws.rows * D);
  ws.nys = a.take<char>(carve_nystrom(&d->attn, ws.rows, nullptr).bytes);
  ws.bytes = a.bytes();
  return ws;
}

// TransMIL.forward for both exports; everything checked by the caller.  attn1 / attn2 (either may be NULL; rw is read only
// when one is not): the cls token's row of layer 1 / layer 2, [heads, 1 + H * H].  Without them the launches are those of
// the plain forward, and logits / feat have the same bits either way (lse is one more store of the landmark merge).
int transmil_forward(const rrt_transmil_desc* desc, const rrt_transmil_weights* w, const float* x, float* logits, float* feat,
                     float* attn1, float* attn2, int64_t n_tokens, const TransmilWs& ws, const RowWs& rw, hipStream_t st) {
  const NystromWs nws = carve_nystrom(&desc->attn, ws.rows, ws.nys);
  const int D = desc->attn.dim, R = (int)ws.rows;
  int rc;
  LinearEpilogue ep{};
  ep.bias = w->fc1_b;
  ep.act = desc->act;
  RRT_TRY(launch_linear(x, w->fc1_w, ws.emb, (int)n_tokens, D, desc->input_dim, ep, st));
  RRT_TRY(launch_transmil_assemble(ws.emb, w->cls_token, ws.seq, (int)n_tokens, R, D, st));
  // layer 1: seq += Nystrom(LN(seq))
  RRT_TRY(launch_layernorm(ws.seq, nullptr, w->layer[0].norm_w, w->layer[0].norm_b, ws.ln, R, D, st));
  rc = nystrom_forward(&desc->attn, &w->layer[0].attn, ws.ln, ws.att, ws.rows, nws, st, attn1 ? rw.lse : nullptr);
  if (!rc && attn1) rc = nystrom_row(&desc->attn, 0, attn1, ws.rows, nws, rw, st);
  if (rc) return rc;
  RRT_TRY(launch_add_cols(ws.seq, ws.att, (size_t)R, D, D, st));
  // PPEG: row 0 passes through
  RRT_TRY(hipMemcpyAsync(ws.seq2, ws.seq, (size_t)D * sizeof(float), hipMemcpyDeviceToDevice, st));
  RRT_TRY(launch_ppeg_side(ws.seq + D, w->pos_w, w->pos_b, ws.seq2 + D, ws.side, D, st));
  // layer 2
  RRT_TRY(launch_layernorm(ws.seq2, nullptr, w->layer[1].norm_w, w->layer[1].norm_b, ws.ln, R, D, st));
  rc = nystrom_forward(&desc->attn, &w->layer[1].attn, ws.ln, ws.att, ws.rows, nws, st, attn2 ? rw.lse : nullptr);
  if (!rc && attn2) rc = nystrom_row(&desc->attn, 0, attn2, ws.rows, nws, rw, st);
  if (rc) return rc;
  RRT_TRY(launch_add_cols(ws.seq2, ws.att, (size_t)R, D, D, st));
  if (feat) RRT_TRY(hipMemcpyAsync(feat, ws.seq2, (size_t)R * D * sizeof(float), hipMemcpyDeviceToDevice, st));
  // the head reads row 0 only
  RRT_TRY(launch_layernorm(ws.seq2, nullptr, w->norm_w, w->norm_b, ws.ln, 1, D, st));
  RRT_TRY(launch_transmil_head(ws.ln, w->fc2_w, w->fc2_b, logits, D, desc->n_classes, st));
  return RRT_OK;
}

bool transmil_weights_ok(const rrt_transmil_desc* desc, const rrt_transmil_weights* w) {
  if (!w->fc1_w || !w->cls_token || !w->norm_w || !w->norm_b || !w->fc2_w || !w->pos_w[0] || !w->pos_w[1] || !w->pos_w[2])
    return false;
  for (int i = 0; i < 2; ++i)
    if (!w->layer[i].norm_w || !w->layer[i].norm_b || !nystrom_weights_ok(&desc->attn, &w->layer[i].attn)) return false;
  return true;
}

// ---- TransMIL: the one-call training step (transmil_bwd.hip; the stages of nystrom.hip / nystrom_bwd.hip, linear_bwd.hip,
// ln_bwd.hip and peg.hip composed on carved structs)
constexpr int DROP_TAG_FC1 = 200, DROP_TAG_ATTN1 = 201, DROP_TAG_ATTN2 = 202;

// tail = false (the step): layer 2 is the full-row forward into att2, of which the head reads row 0.  tail = true (the
// rrt_debug_transmil_*_row twins, the other side of tools/bench_transmil_train.py's A/B): layer 2 runs its output stage and
// to_out for the cls row alone, and its attention stash holds no o
struct TransmilStash {
  float *hpre, *seq0, *ln1, *seq1, *seq2, *ln2, *hrow, *stats, *orow, *yrow, *att2;
  float* emb;        // forward scratch: the place of ln1, which is written after emb has been read
  char *nys1, *nys2;
  int64_t rows;
  int side;
  size_t bytes;
};
TransmilStash carve_transmil_stash(const rrt_transmil_desc* d, int64_t N, char* base, bool tail) {
  TransmilStash s{};
  s.side = ceil_sqrt_i64(N);
  s.rows = 1 + (int64_t)s.side * s.side;
  const size_t D = (size_t)d->attn.dim, RD = (size_t)s.rows * D;
  Arena a{base};
  if (d->act != RRT_ACT_NONE) s.hpre = a.take((size_t)N * D);
  s.seq0 = a.take(RD);
  s.ln1 = a.take(RD);
  s.emb = s.ln1;
  s.seq1 = a.take(RD);
  s.seq2 = a.take(RD);
  s.ln2 = a.take(RD);
  s.hrow = a.take(D);
  s.stats = a.take(2);
  s.orow = a.take((size_t)d->attn.heads * 64);
  s.yrow = a.take(D);
  s.nys1 = a.take<char>(carve_nystrom_stash(&d->attn, s.rows, nullptr).bytes);
  s.nys2 = a.take<char>(carve_nystrom_stash(&d->attn, s.rows, nullptr, !tail).bytes);
  if (!tail) s.att2 = a.take(RD);
  s.bytes = a.bytes();
  return s;
}

struct TransmilBwdWs {
  float *dgb, *d_hrow, *d_yrow, *d_orow, *A, *B, *C;
  char *nys, *lnp, *ppeg, *lin;
  size_t bytes;
};
TransmilBwdWs carve_transmil_bwd(const rrt_transmil_desc* d, int64_t N, char* base) {
  TransmilBwdWs ws{};
  const int side = ceil_sqrt_i64(N);
  const int64_t rows = 1 + (int64_t)side * side;
  const size_t D = (size_t)d->attn.dim, RD = (size_t)rows * D;
  Arena a{base};
  ws.dgb = a.take(2 * D);
  ws.d_hrow = a.take(D);
  ws.d_yrow = a.take(D);
  ws.d_orow = a.take((size_t)d->attn.heads * 64);
  ws.A = a.take(RD);
  ws.B = a.take(RD);
  ws.C = a.take(RD);
  ws.nys = a.take<char>(carve_nystrom_bwd(&d->attn, rows, nullptr).bytes);
  ws.lnp = a.take<char>(ln_bwd_workspace((int)D));
  ws.ppeg = a.take<char>(ppeg_side_bwd_workspace(side, (int)D));
  ws.lin = a.take<char>(linear_bwd_workspace((int)N, (int)D, d->input_dim));
  ws.bytes = a.bytes();
  return ws;
}

bool transmil_grads_ok(const rrt_transmil_desc* desc, const rrt_transmil_grads* g) {
  if (!g->fc1_w || !g->fc1_b || !g->cls_token || !g->norm_w || !g->norm_b || !g->fc2_w || !g->fc2_b) return false;
  for (int i = 0; i < 3; ++i)
    if (!g->pos_w[i] || !g->pos_b[i]) return false;
  for (int i = 0; i < 2; ++i) {
    const rrt_transmil_layer_grads& l = g->layer[i];
    if (!l.norm_w || !l.norm_b || !l.attn.qkv_w || !l.attn.out_w || !l.attn.out_b || (desc->attn.residual && !l.attn.conv_w))
      return false;
  }
  return true;
}

// arguments of both calls that are checked the same way; fills the two mask configurations
int check_transmil_step(const rrt_transmil_desc* desc, const rrt_transmil_weights* w, int64_t n_tokens, float fc1_drop_p,
                        float attn_drop_p, DropCfg* d1, DropCfg* da) {
  int rc = check_transmil(desc, n_tokens);
  if (rc) return rc;
  if (!transmil_weights_ok(desc, w) || !w->fc1_b || !w->fc2_b || !w->pos_b[0] || !w->pos_b[1] || !w->pos_b[2]) return RRT_E_INVALID;
  if (make_drop(fc1_drop_p, d1) || make_drop(attn_drop_p, da)) return RRT_E_INVALID;
  return RRT_OK;
}

int transmil_forward_train(const rrt_transmil_desc* desc, const rrt_transmil_weights* w, const float* x, float* logits,
                           int64_t N, const TransmilStash& S, const DropCfg& d1, const DropCfg& da, uint64_t seed, bool tail,
                           hipStream_t st) {
  const rrt_nystrom_desc* ad = &desc->attn;
  const NystromStash s1 = carve_nystrom_stash(ad, S.rows, S.nys1), s2 = carve_nystrom_stash(ad, S.rows, S.nys2, !tail);
  const int D = ad->dim, R = (int)S.rows, hd = ad->heads * 64;
  int rc;
  // _fc1: Linear (+ activation as a pass over the kept pre-activation) + Dropout
  LinearEpilogue ep{};
  ep.bias = w->fc1_b;
  if (desc->act != RRT_ACT_NONE) {
    RRT_TRY(launch_linear(x, w->fc1_w, S.hpre, (int)N, D, desc->input_dim, ep, st));
    RRT_TRY(launch_act_forward(S.hpre, S.emb, (size_t)N * D, desc->act, d1.thresh, d1.seed(seed, DROP_TAG_FC1), d1.scale, st));
  } else {
    RRT_TRY(launch_linear(x, w->fc1_w, S.emb, (int)N, D, desc->input_dim, ep, st));
    RRT_TRY(launch_apply_drop_mask(S.emb, (int)N, D, d1.thresh, d1.seed(seed, DROP_TAG_FC1), d1.scale, st));
  }
  RRT_TRY(launch_transmil_assemble(S.emb, w->cls_token, S.seq0, (int)N, R, D, st));
  // layer 1: seq1 = seq0 + drop(Nystrom(LN(seq0)))
  RRT_TRY(launch_layernorm(S.seq0, nullptr, w->layer[0].norm_w, w->layer[0].norm_b, S.ln1, R, D, st));
  rc = nystrom_forward(ad, &w->layer[0].attn, S.ln1, S.seq1, S.rows, s1.f, st, s1.lse);
  if (rc) return rc;
  RRT_TRY(launch_apply_drop_mask(S.seq1, R, D, da.thresh, da.seed(seed, DROP_TAG_ATTN1), da.scale, st));
  RRT_TRY(launch_add_cols(S.seq1, S.seq0, (size_t)R, D, D, st));
  // PPEG: row 0 passes through
  RRT_TRY(hipMemcpyAsync(S.seq2, S.seq1, (size_t)D * sizeof(float), hipMemcpyDeviceToDevice, st));
  RRT_TRY(launch_ppeg_side(S.seq1 + D, w->pos_w, w->pos_b, S.seq2 + D, S.side, D, st));
  // layer 2: only row 0 of seq2 + drop(Nystrom(LN(seq2))) is read
  RRT_TRY(launch_layernorm(S.seq2, nullptr, w->layer[1].norm_w, w->layer[1].norm_b, S.ln2, R, D, st));
  const float* yrow = S.yrow;
  if (tail) {
    rc = nystrom_front(ad, &w->layer[1].attn, S.ln2, S.rows, s2.f, st, s2.lse);
    if (rc) return rc;
    RRT_TRY(launch_nystrom_output_row(s2.f.qkv, s2.f.kl, s2.f.wz, ad->residual ? w->layer[1].attn.conv_w : nullptr, S.orow,
                                      (long)(s2.f.np - S.rows), (long)s2.f.np, ad->heads, ad->residual_conv_kernel, st));
    RRT_TRY(launch_row_linear(S.orow, w->layer[1].attn.out_w, w->layer[1].attn.out_b, S.yrow, D, hd, st));
  } else {
    rc = nystrom_forward(ad, &w->layer[1].attn, S.ln2, S.att2, S.rows, s2.f, st, s2.lse);
    if (rc) return rc;
    yrow = S.att2;
  }
  // mask + residual on row 0, the last LayerNorm, _fc2
  RRT_TRY(launch_transmil_row_head(S.seq2, yrow, w->norm_w, w->norm_b, w->fc2_w, w->fc2_b, S.hrow, S.stats, logits, D,
                                   desc->n_classes, da.thresh, da.seed(seed, DROP_TAG_ATTN2), da.scale, st));
  return RRT_OK;
}

int transmil_backward(const rrt_transmil_desc* desc, const rrt_transmil_weights* w, const float* x, const float* d_logits,
                      const TransmilStash& S, const TransmilBwdWs& W, const rrt_transmil_grads* g, float* dx, int64_t N,
                      const DropCfg& d1, const DropCfg& da, uint64_t seed, bool tail, hipStream_t st) {
  const rrt_nystrom_desc* ad = &desc->attn;
  const NystromStash s1 = carve_nystrom_stash(ad, S.rows, S.nys1), s2 = carve_nystrom_stash(ad, S.rows, S.nys2, !tail);
  const NystromBwdWs nb = carve_nystrom_bwd(ad, S.rows, W.nys);
  const int D = ad->dim, R = (int)S.rows, hd = ad->heads * 64;
  const size_t row_bytes = (size_t)D * sizeof(float);
  int rc;
  // the head: _fc2, the last LayerNorm, and the one nonzero row of layer 2's output cotangent
  RRT_TRY(launch_transmil_row_head_backward(d_logits, S.hrow, S.stats, w->norm_w, w->norm_b, w->fc2_w, g->fc2_w, g->fc2_b,
                                            g->norm_w, g->norm_b, W.d_hrow, W.d_yrow, D, desc->n_classes, da.thresh,
                                            da.seed(seed, DROP_TAG_ATTN2), da.scale, st));
  // layer 2's attention -> A = d ln2
  const rrt_nystrom_grads* g2 = &g->layer[1].attn;
  if (tail) {
    RRT_TRY(launch_row_linear_backward(W.d_yrow, S.orow, w->layer[1].attn.out_w, g2->out_w, g2->out_b, W.d_orow, D, hd, st));
    RRT_TRY(launch_nystrom_output_row_backward(s2.f.qkv, s2.f.kl, s2.f.wz, ad->residual ? w->layer[1].attn.conv_w : nullptr,
                                               W.d_orow, nb.d_qkv, nb.d_kl, nb.d_wz, g2->conv_w, (long)(s2.f.np - S.rows),
                                               (long)s2.f.np, ad->heads, ad->residual_conv_kernel, st));
    rc = nystrom_backward_rest(ad, &w->layer[1].attn, S.ln2, s2, nb, g2, W.A, S.rows, st);
  } else {
    RRT_TRY(hipMemsetAsync(W.C, 0, (size_t)R * row_bytes, st));
    RRT_TRY(hipMemcpyAsync(W.C, W.d_yrow, row_bytes, hipMemcpyDeviceToDevice, st));
    rc = nystrom_backward(ad, &w->layer[1].attn, S.ln2, W.C, s2, nb, g2, W.A, S.rows, st);
  }
  if (rc) return rc;
  // LayerNorm 2 -> B = d seq2; the residual reaches row 0 alone
  RRT_TRY(launch_ln_backward(W.A, S.seq2, w->layer[1].norm_w, nullptr, W.B, W.dgb, (float*)W.lnp, R, D, nullptr, st));
  RRT_TRY(hipMemcpyAsync(g->layer[1].norm_w, W.dgb, row_bytes, hipMemcpyDeviceToDevice, st));
  RRT_TRY(hipMemcpyAsync(g->layer[1].norm_b, W.dgb + D, row_bytes, hipMemcpyDeviceToDevice, st));
  RRT_TRY(launch_add_cols(W.B, W.d_hrow, 1, D, D, st));
  // PPEG -> A = d seq1 (row 0 passes through)
  RRT_TRY(hipMemcpyAsync(W.A, W.B, row_bytes, hipMemcpyDeviceToDevice, st));
  RRT_TRY(launch_ppeg_side_backward(S.seq1 + D, W.B + D, w->pos_w, W.A + D, g->pos_w, g->pos_b, S.side, D, W.ppeg, st));
  // layer 1: the attention branch under its mask -> B = d ln1; LayerNorm 1 with the residual branch -> C = d seq0
  const float* dy1 = W.A;
  if (da.thresh) {
    RRT_TRY(launch_copy_drop_mask(W.A, W.C, (size_t)R * D, da.thresh, da.seed(seed, DROP_TAG_ATTN1), da.scale, st));
    dy1 = W.C;
  }
  rc = nystrom_backward(ad, &w->layer[0].attn, S.ln1, dy1, s1, nb, &g->layer[0].attn, W.B, S.rows, st);
  if (rc) return rc;
  RRT_TRY(launch_ln_backward(W.B, S.seq0, w->layer[0].norm_w, W.A, W.C, W.dgb, (float*)W.lnp, R, D, nullptr, st));
  RRT_TRY(hipMemcpyAsync(g->layer[0].norm_w, W.dgb, row_bytes, hipMemcpyDeviceToDevice, st));
  RRT_TRY(hipMemcpyAsync(g->layer[0].norm_b, W.dgb + D, row_bytes, hipMemcpyDeviceToDevice, st));
  // the assembly, _fc1's mask and activation -> A = d (_fc1.0's output); then _fc1.0 (dx == NULL: no dX product)
  RRT_TRY(launch_transmil_assemble_backward(W.C, S.hpre, W.A, g->cls_token, (int)N, S.side, D, desc->act, d1.thresh,
                                            d1.seed(seed, DROP_TAG_FC1), d1.scale, st));
  RRT_TRY(launch_linear_backward(W.A, x, w->fc1_w, dx, g->fc1_w, g->fc1_b, (int)N, D, desc->input_dim, RRT_COMPUTE_F32, W.lin,
                                 st));
  return RRT_OK;
}

int transmil_train_sizes(const rrt_transmil_desc* desc, int64_t n_tokens, size_t* stash_bytes, size_t* bwd_bytes, bool tail) {
  if (!stash_bytes || !bwd_bytes) return RRT_E_INVALID;
  int rc = check_transmil(desc, n_tokens);
  if (rc) return rc;
  *stash_bytes = carve_transmil_stash(desc, n_tokens, nullptr, tail).bytes;
  *bwd_bytes = carve_transmil_bwd(desc, n_tokens, nullptr).bytes;
  return RRT_OK;
}

int transmil_forward_train_entry(const rrt_transmil_desc* desc, const rrt_transmil_weights* w, const float* x, float* logits,
                                 int64_t n_tokens, void* stash, size_t stash_bytes, float fc1_drop_p, float attn_drop_p,
                                 uint64_t drop_seed, void* stream, bool tail) {
  if (!desc || !w || !x || !logits) return RRT_E_INVALID;
  DropCfg d1{}, da{};
  int rc = check_transmil_step(desc, w, n_tokens, fc1_drop_p, attn_drop_p, &d1, &da);
  if (rc) return rc;
  if (!stash || stash_bytes < carve_transmil_stash(desc, n_tokens, nullptr, tail).bytes) return RRT_E_WORKSPACE;
  return transmil_forward_train(desc, w, x, logits, n_tokens, carve_transmil_stash(desc, n_tokens, (char*)stash, tail), d1, da,
                                drop_seed, tail, (hipStream_t)stream);
}

int transmil_backward_entry(const rrt_transmil_desc* desc, const rrt_transmil_weights* w, const float* x, const float* d_logits,
                            const void* stash, size_t stash_bytes, const rrt_transmil_grads* grads, float* dx, int64_t n_tokens,
                            void* workspace, size_t workspace_bytes, float fc1_drop_p, float attn_drop_p, uint64_t drop_seed,
                            void* stream, bool tail) {
  if (!desc || !w || !x || !d_logits || !grads) return RRT_E_INVALID;
  DropCfg d1{}, da{};
  int rc = check_transmil_step(desc, w, n_tokens, fc1_drop_p, attn_drop_p, &d1, &da);
  if (rc) return rc;
  if (!transmil_grads_ok(desc, grads)) return RRT_E_INVALID;
  if (!stash || stash_bytes < carve_transmil_stash(desc, n_tokens, nullptr, tail).bytes) return RRT_E_WORKSPACE;
  if (!workspace || workspace_bytes < carve_transmil_bwd(desc, n_tokens, nullptr).bytes) return RRT_E_WORKSPACE;
  return transmil_backward(desc, w, x, d_logits, carve_transmil_stash(desc, n_tokens, (char*)stash, tail),
                           carve_transmil_bwd(desc, n_tokens, (char*)workspace), grads, dx, n_tokens, d1, da, drop_seed, tail,
                           (hipStream_t)stream);
}

// ---- the Nystrom ablations of RRTEncoder (modules/rrt.py:49-58, modules/rmsa.py:167-230)
int check_encoder_nystrom(const rrt_encoder_desc* d, const rrt_encoder_nystrom_desc* nys, int64_t N, rrt_grid* g) {
  if (!d || !nys || N <= 0) return RRT_E_INVALID;
  if (nys->mode != RRT_NYSTROM_BAG && nys->mode != RRT_NYSTROM_REGIONS)
    return unsupported("encoder_nystrom: mode must be RRT_NYSTROM_BAG or RRT_NYSTROM_REGIONS");
  if (d->compute != RRT_COMPUTE_F32) return unsupported("encoder_nystrom: compute must be RRT_COMPUTE_F32 (exact fp32 only)");
  if (d->n_rmsa_layers < 1 || d->n_rmsa_layers > RRT_MAX_RMSA_LAYERS) return unsupported("encoder_nystrom: n_rmsa_layers out of range");
  if (nys->attn.dim != d->dim) return unsupported("encoder_nystrom: attn.dim must be the encoder's dim");
  if (N > 1000000) return unsupported("encoder_nystrom: n_tokens above 1e6");
  *g = rrt_grid{};
  int64_t n = N;
  if (nys->mode == RRT_NYSTROM_REGIONS) {
    int rc = rrt_region_grid(N, d->region_num, d->region_size, d->min_region_num, d->min_region_ratio, g);
    if (rc) return rc == RRT_E_INVALID && d->region_size <= 0 && d->region_num <= 0 ? unsupported("region_num must be positive") : rc;
    n = (int64_t)g->s * g->s;
    rc = check_nystrom_batch((int64_t)g->regions_side * g->regions_side);
    if (rc) return rc;
  }
  int rc = check_nystrom(&nys->attn, n);
  if (rc) return rc;
  if (nys->attn.heads * nys->attn.dim_head != d->dim) return unsupported("encoder_nystrom: attn.heads * attn.dim_head must equal dim");
  if (d->pos) {
    if (d->pos != RRT_POS_PEG && d->pos != RRT_POS_PPEG) return unsupported("pos must be none / peg / ppeg");
    if (d->peg_k <= 0 || d->peg_k % 2 == 0 || d->peg_k > 11) return unsupported("peg_k must be odd and <= 11");
    if (d->pos_pos != -1 && d->pos_pos != 0) return unsupported("pos_pos must be -1 or 0");
  }
  if (d->ffn) {
    if (d->ffn_hidden <= 0 || d->ffn_hidden % 32 != 0)
      return unsupported("ffn: hidden width int(dim * mlp_ratio) must be a positive multiple of 32");
    if (d->ffn_act != RRT_ACT_GELU && d->ffn_act != RRT_ACT_RELU) return unsupported("ffn_act must be gelu or relu");
  }
  return RRT_OK;
}

struct EncoderNystromWs {
  char *tail, *nys;
  float *xa, *xb, *u, *att, *hid;
  size_t tail_bytes, bytes;
};
EncoderNystromWs carve_encoder_nystrom(const rrt_encoder_desc* d, const rrt_encoder_nystrom_desc* nys, int64_t N, const rrt_grid& g,
                                       size_t tail_bytes, char* base) {
  EncoderNystromWs ws{};
  const size_t D = (size_t)d->dim;
  const bool regions = nys->mode == RRT_NYSTROM_REGIONS;
  const size_t Np = regions ? (size_t)g.H * g.H : (size_t)N;
  Arena a{base};
  ws.tail = a.take<char>(tail_bytes);
  ws.tail_bytes = tail_bytes;
  ws.xa = a.take((size_t)N * D);
  ws.xb = a.take((size_t)N * D);
  ws.u = a.take(Np * D);               // LN(x) (region mode: partitioned, its appended rows zero)
  ws.att = a.take((size_t)N * D);      // an attention's or an FFN's output in front of its residual
  if (d->ffn) ws.hid = a.take((size_t)N * d->ffn_hidden);
  ws.nys = a.take<char>(regions ? carve_nystrom(&nys->attn, (int64_t)g.s * g.s, nullptr, true, (int64_t)g.regions_side * g.regions_side).bytes
                                : carve_nystrom(&nys->attn, N, nullptr).bytes);
  ws.bytes = a.bytes();
  return ws;
}

// everything checked by the caller.  cur is the activations' own buffer (xa or xb): the residuals are added in place, a stage
// that cannot run in place writes the other buffer.
int encoder_nystrom_forward(const rrt_encoder_desc* desc, const rrt_encoder_nystrom_desc* nys, const rrt_encoder_weights* w,
                            const float* x, float* y, int64_t N, const rrt_grid& g, const EncoderNystromWs& ws, hipStream_t st) {
  const rrt_nystrom_desc* ad = &nys->attn;
  const int D = desc->dim;
  const bool regions = nys->mode == RRT_NYSTROM_REGIONS;
  float* cur = ws.xa;
  float* other = ws.xb;
  auto swap = [&]() {
    float* t = cur;
    cur = other;
    other = t;
  };
  auto pos_embed = [&](const float* in, float* out) -> int {
    if (!w->pos_w[0] || (desc->pos == RRT_POS_PPEG && (!w->pos_w[1] || !w->pos_w[2]))) return RRT_E_INVALID;
    RRT_TRY(launch_peg(in, w->pos_w, w->pos_b, out, (int)N, D, desc->peg_k, desc->peg_1d, desc->pos == RRT_POS_PPEG, st));
    return RRT_OK;
  };
  int rc;
  if (desc->pos && desc->pos_pos == -1) {
    rc = pos_embed(x, cur);
    if (rc) return rc;
  } else {
    RRT_TRY(hipMemcpyAsync(cur, x, (size_t)N * D * sizeof(float), hipMemcpyDeviceToDevice, st));
  }
  for (int li = 0; li < desc->n_rmsa_layers; ++li) {
    if (li == 1 && desc->pos && desc->pos_pos == 0) {
      rc = pos_embed(cur, other);
      if (rc) return rc;
      swap();
    }
    const rrt_attn_weights& lw = w->rmsa[li];
    if (!lw.norm_w || !lw.norm_b) return RRT_E_INVALID;
    rrt_nystrom_weights aw{lw.qkv_w, lw.proj_w, lw.proj_b, lw.pe_w};
    if (!nystrom_weights_ok(ad, &aw)) return RRT_E_INVALID;
    if (!regions) {
      // x += NystromAttention(LN(x)) over the whole bag
      RRT_TRY(launch_layernorm(cur, nullptr, lw.norm_w, lw.norm_b, ws.u, (int)N, D, st));
      rc = nystrom_forward(ad, &aw, ws.u, ws.att, N, carve_nystrom(ad, N, ws.nys), st);
      if (rc) return rc;
      RRT_TRY(launch_add_cols(cur, ws.att, (size_t)N, D, D, st));
    } else {
      // LN + zero rows to H * H + partition -> u [R, P, D]; the attention over the R regions; to_out with the un-partition,
      // the drop of the appended rows and the residual in its epilogue (slot -> token, as R-MSA's out-projection)
      const GridDev gd = to_dev(g);
      const int64_t R = gd.Rt, P = gd.P;
      const NystromWs nws = carve_nystrom(ad, P, ws.nys, true, R);
      RRT_TRY(launch_ln_partition(cur, lw.norm_w, lw.norm_b, ws.u, D, gd, st));
      const float* o = nullptr;
      if (R == 1) {
        // one region: the single-sequence stages; its output rows are the padded buffer's last P
        rc = nystrom_front(ad, &aw, ws.u, P, nws, st, nullptr);
        if (rc) return rc;
        RRT_TRY(launch_nystrom_output(nws.qkv, nws.kl, nws.wz, ad->residual ? aw.conv_w : nullptr, nws.o, (long)nws.np, ad->heads,
                                      ad->residual_conv_kernel, st));
        o = nws.o + (size_t)(nws.np - P) * D;
      } else {
        rc = nystrom_batched_front(ad, &aw, ws.u, P, nws, st, &o);
        if (rc) return rc;
      }
      LinearEpilogue ep{};
      ep.bias = aw.out_b;
      ep.resid = cur;
      ep.g = gd;
      RRT_TRY(launch_linear(o, aw.out_w, other, gd.Np, D, D, ep, st));
      swap();
    }
    if (desc->ffn) {
      // x += fc2(act(fc1(LN2(x))))
      if (!lw.norm2_w || !lw.norm2_b || !lw.fc1_w || !lw.fc1_b || !lw.fc2_w || !lw.fc2_b) return RRT_E_INVALID;
      RRT_TRY(launch_layernorm(cur, nullptr, lw.norm2_w, lw.norm2_b, ws.u, (int)N, D, st));
      LinearEpilogue e1{};
      e1.bias = lw.fc1_b;
      e1.act = desc->ffn_act;
      RRT_TRY(launch_linear(ws.u, lw.fc1_w, ws.hid, (int)N, desc->ffn_hidden, D, e1, st));
      LinearEpilogue e2{};
      e2.bias = lw.fc2_b;
      RRT_TRY(launch_linear(ws.hid, lw.fc2_w, ws.att, (int)N, D, desc->ffn_hidden, e2, st));
      RRT_TRY(launch_add_cols(cur, ws.att, (size_t)N, D, D, st));
    }
  }
  return encoder_tail(desc, w, cur, x, y, N, ws.tail, ws.tail_bytes, st);
}
}  // namespace

extern "C" {
// ---- Nystrom attention: the forward, its stages and one query row of the approximated attention matrix
int rrt_nystrom_workspace_size(const rrt_nystrom_desc* desc, int64_t n, size_t* bytes) {
  if (!bytes) return RRT_E_INVALID;
  int rc = check_nystrom(desc, n);
  if (rc) return rc;
  *bytes = carve_nystrom(desc, n, nullptr).bytes;
  return RRT_OK;
}

int rrt_nystrom_attention_f32(const rrt_nystrom_desc* desc, const rrt_nystrom_weights* w, const float* x, float* y, int64_t n,
                              void* workspace, size_t workspace_bytes, void* stream) {
  if (!desc || !w || !x || !y) return RRT_E_INVALID;
  int rc = check_nystrom(desc, n);
  if (rc) return rc;
  if (!nystrom_weights_ok(desc, w)) return RRT_E_INVALID;
  if (!workspace || workspace_bytes < carve_nystrom(desc, n, nullptr).bytes) return RRT_E_WORKSPACE;
  return nystrom_forward(desc, w, x, y, n, carve_nystrom(desc, n, (char*)workspace), (hipStream_t)stream);
}

int rrt_nystrom_landmarks_f32(const float* qkv, float* ql, float* kl, int64_t n_padded, int32_t heads, void* stream) {
  if (!qkv || !ql || !kl) return RRT_E_INVALID;
  int rc = check_nystrom_np(n_padded);
  if (!rc) rc = check_nystrom_heads(heads);
  if (rc) return rc;
  return (int)launch_nystrom_landmarks(qkv, ql, kl, (long)n_padded, heads, (hipStream_t)stream);
}

int rrt_nystrom_landmark_sim_f32(const float* ql, const float* kl, float* a2, int32_t heads, void* stream) {
  if (!ql || !kl || !a2) return RRT_E_INVALID;
  int rc = check_nystrom_heads(heads);
  if (rc) return rc;
  return (int)launch_nystrom_sim2(ql, kl, a2, heads, (hipStream_t)stream);
}

int rrt_nystrom_landmark_attn_workspace_size(int64_t n_padded, int32_t heads, size_t* bytes) {
  if (!bytes) return RRT_E_INVALID;
  int rc = check_nystrom_np(n_padded);
  if (!rc) rc = check_nystrom_heads(heads);
  if (rc) return rc;
  *bytes = nystrom_lattn_floats((long)n_padded, heads) * sizeof(float);
  return RRT_OK;
}

int rrt_nystrom_landmark_attn_f32(const float* qkv, const float* ql, float* av, int64_t n_padded, int32_t heads,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  if (!qkv || !ql || !av) return RRT_E_INVALID;
  int rc = check_nystrom_np(n_padded);
  if (!rc) rc = check_nystrom_heads(heads);
  if (rc) return rc;
  if (!workspace || workspace_bytes < nystrom_lattn_floats((long)n_padded, heads) * sizeof(float)) return RRT_E_WORKSPACE;
  return (int)launch_nystrom_lattn(qkv, ql, av, (float*)workspace, (long)n_padded, heads, (hipStream_t)stream);
}

int rrt_nystrom_pinv_workspace_size(int32_t heads, size_t* bytes) {
  if (!bytes) return RRT_E_INVALID;
  int rc = check_nystrom_heads(heads);
  if (rc) return rc;
  *bytes = nystrom_pinv_floats(heads) * sizeof(float);
  return RRT_OK;
}

int rrt_nystrom_pinv_f32(const float* a2, float* z, int32_t heads, int32_t iterations, void* workspace, size_t workspace_bytes,
                         void* stream) {
  if (!a2 || !z) return RRT_E_INVALID;
  int rc = check_nystrom_heads(heads);
  if (rc) return rc;
  if (iterations < 1 || iterations > 16) return unsupported("nystrom: pinv_iterations must be in 1..16");
  if (!workspace || workspace_bytes < nystrom_pinv_floats(heads) * sizeof(float)) return RRT_E_WORKSPACE;
  return (int)launch_nystrom_pinv(a2, z, (float*)workspace, heads, iterations, (hipStream_t)stream);
}

int rrt_nystrom_zav_f32(const float* z, const float* av, float* wz, int32_t heads, void* stream) {
  if (!z || !av || !wz) return RRT_E_INVALID;
  int rc = check_nystrom_heads(heads);
  if (rc) return rc;
  return (int)launch_nystrom_zav(z, av, wz, heads, (hipStream_t)stream);
}

int rrt_nystrom_output_f32(const float* qkv, const float* kl, const float* wz, const float* conv_w, float* o, int64_t n_padded,
                           int32_t heads, int32_t conv_k, void* stream) {
  if (!qkv || !kl || !wz || !o) return RRT_E_INVALID;
  int rc = check_nystrom_np(n_padded);
  if (!rc) rc = check_nystrom_heads(heads);
  if (rc) return rc;
  if (conv_w && (conv_k < 1 || conv_k % 2 == 0 || conv_k > 63)) return unsupported("nystrom: residual_conv_kernel must be odd and <= 63");
  return (int)launch_nystrom_output(qkv, kl, wz, conv_w, o, (long)n_padded, heads, conv_k, (hipStream_t)stream);
}

int rrt_nystrom_attn_row_f32(const float* qkv, const float* ql, const float* kl, const float* z, const float* lse3, float* r,
                             float* attn, int64_t row_padded, int64_t n_padded, int32_t heads, void* stream) {
  if (!qkv || !ql || !kl || !z || !lse3 || !r || !attn) return RRT_E_INVALID;
  int rc = check_nystrom_np(n_padded);
  if (!rc) rc = check_nystrom_heads(heads);
  if (rc) return rc;
  if (row_padded < 0 || row_padded >= n_padded) return unsupported("nystrom: row_padded must be in [0, n_padded)");
  return (int)launch_nystrom_attn_row(qkv, ql, kl, z, lse3, r, attn, (long)row_padded, (long)n_padded, 0, (long)n_padded, heads,
                                      (hipStream_t)stream);
}

int rrt_nystrom_attention_row_workspace_size(const rrt_nystrom_desc* desc, int64_t n, size_t* bytes) {
  if (!bytes) return RRT_E_INVALID;
  int rc = check_nystrom(desc, n);
  if (rc) return rc;
  *bytes = carve_row(carve_nystrom(desc, n, nullptr).bytes, desc->heads, nullptr).bytes;
  return RRT_OK;
}

int rrt_nystrom_attention_row_f32(const rrt_nystrom_desc* desc, const rrt_nystrom_weights* w, const float* x, float* y,
                                  int64_t row, float* attn, int64_t n, void* workspace, size_t workspace_bytes, void* stream) {
  if (!desc || !w || !x || !y || !attn) return RRT_E_INVALID;
  int rc = check_nystrom(desc, n);
  if (rc) return rc;
  if (!nystrom_weights_ok(desc, w)) return RRT_E_INVALID;
  if (row < 0 || row >= n) return unsupported("nystrom: row must be in [0, n)");
  const size_t front = carve_nystrom(desc, n, nullptr).bytes;
  if (!workspace || workspace_bytes < carve_row(front, desc->heads, nullptr).bytes) return RRT_E_WORKSPACE;
  const NystromWs ws = carve_nystrom(desc, n, (char*)workspace);
  const RowWs rw = carve_row(front, desc->heads, (char*)workspace);
  rc = nystrom_forward(desc, w, x, y, n, ws, (hipStream_t)stream, rw.lse);
  if (rc) return rc;
  return nystrom_row(desc, row, attn, n, ws, rw, (hipStream_t)stream);
}

// ---- ... b sequences per launch: the forward and its stages (the b = 1 calls are the single-sequence ones, launch for launch)
int rrt_nystrom_batched_workspace_size(const rrt_nystrom_desc* desc, int64_t b, int64_t n, size_t* bytes) {
  if (!bytes) return RRT_E_INVALID;
  int rc = check_nystrom(desc, n);
  if (!rc) rc = check_nystrom_batch(b);
  if (!rc) rc = check_nystrom_rows(b, n);
  if (rc) return rc;
  *bytes = carve_nystrom(desc, n, nullptr, true, b).bytes;
  return RRT_OK;
}

int rrt_nystrom_attention_batched_f32(const rrt_nystrom_desc* desc, const rrt_nystrom_weights* w, const float* x, float* y,
                                      int64_t b, int64_t n, void* workspace, size_t workspace_bytes, void* stream) {
  if (!desc || !w || !x || !y) return RRT_E_INVALID;
  int rc = check_nystrom(desc, n);
  if (!rc) rc = check_nystrom_batch(b);
  if (!rc) rc = check_nystrom_rows(b, n);
  if (rc) return rc;
  if (!nystrom_weights_ok(desc, w)) return RRT_E_INVALID;
  if (!workspace || workspace_bytes < carve_nystrom(desc, n, nullptr, true, b).bytes) return RRT_E_WORKSPACE;
  const NystromWs ws = carve_nystrom(desc, n, (char*)workspace, true, b);
  hipStream_t st = (hipStream_t)stream;
  if (b == 1) return nystrom_forward(desc, w, x, y, n, ws, st);
  const float* o = nullptr;
  rc = nystrom_batched_front(desc, w, x, n, ws, st, &o);
  if (rc) return rc;
  LinearEpilogue eo{};
  eo.bias = w->out_b;
  RRT_TRY(launch_linear(o, w->out_w, y, (int)(b * n), desc->dim, desc->heads * 64, eo, st));
  return RRT_OK;
}

int rrt_nystrom_landmarks_batched_f32(const float* qkv, float* ql, float* kl, int64_t b, int64_t n_padded, int32_t heads,
                                      void* stream) {
  if (!qkv || !ql || !kl) return RRT_E_INVALID;
  int rc = check_np_heads(n_padded, heads);
  if (!rc) rc = check_nystrom_batch(b);
  if (rc) return rc;
  return (int)launch_nystrom_landmarks(qkv, ql, kl, (long)n_padded, heads, (hipStream_t)stream, (int)b);
}

int rrt_nystrom_landmark_sim_batched_f32(const float* ql, const float* kl, float* a2, int64_t b, int32_t heads, void* stream) {
  if (!ql || !kl || !a2) return RRT_E_INVALID;
  int rc = check_nystrom_heads(heads);
  if (!rc) rc = check_nystrom_batch(b);
  if (rc) return rc;
  return (int)launch_nystrom_sim2(ql, kl, a2, heads, (hipStream_t)stream, (int)b);
}

int rrt_nystrom_landmark_attn_batched_workspace_size(int64_t b, int64_t n_padded, int32_t heads, size_t* bytes) {
  if (!bytes) return RRT_E_INVALID;
  int rc = check_np_heads(n_padded, heads);
  if (!rc) rc = check_nystrom_batch(b);
  if (rc) return rc;
  *bytes = nystrom_lattn_floats((long)n_padded, heads, (int)b) * sizeof(float);
  return RRT_OK;
}

int rrt_nystrom_landmark_attn_batched_f32(const float* qkv, const float* ql, float* av, int64_t b, int64_t n_padded,
                                          int32_t heads, void* workspace, size_t workspace_bytes, void* stream) {
  if (!qkv || !ql || !av) return RRT_E_INVALID;
  int rc = check_np_heads(n_padded, heads);
  if (!rc) rc = check_nystrom_batch(b);
  if (rc) return rc;
  if (!workspace || workspace_bytes < nystrom_lattn_floats((long)n_padded, heads, (int)b) * sizeof(float)) return RRT_E_WORKSPACE;
  return (int)launch_nystrom_lattn(qkv, ql, av, (float*)workspace, (long)n_padded, heads, (hipStream_t)stream, nullptr, (int)b);
}

int rrt_nystrom_pinv_batched_workspace_size(int64_t b, int32_t heads, size_t* bytes) {
  if (!bytes) return RRT_E_INVALID;
  int rc = check_nystrom_heads(heads);
  if (!rc) rc = check_nystrom_batch(b);
  if (rc) return rc;
  *bytes = nystrom_pinv_floats(heads, (int)b) * sizeof(float);
  return RRT_OK;
}

int rrt_nystrom_pinv_batched_f32(const float* a2, float* z, int64_t b, int32_t heads, int32_t iterations, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  if (!a2 || !z) return RRT_E_INVALID;
  int rc = check_nystrom_heads(heads);
  if (!rc) rc = check_pinv_iterations(iterations);
  if (!rc) rc = check_nystrom_batch(b);
  if (rc) return rc;
  if (!workspace || workspace_bytes < nystrom_pinv_floats(heads, (int)b) * sizeof(float)) return RRT_E_WORKSPACE;
  return (int)launch_nystrom_pinv(a2, z, (float*)workspace, heads, iterations, (hipStream_t)stream, (int)b);
}

int rrt_nystrom_zav_batched_f32(const float* z, const float* av, float* wz, int64_t b, int32_t heads, void* stream) {
  if (!z || !av || !wz) return RRT_E_INVALID;
  int rc = check_nystrom_heads(heads);
  if (!rc) rc = check_nystrom_batch(b);
  if (rc) return rc;
  return (int)launch_nystrom_zav(z, av, wz, heads, (hipStream_t)stream, (int)b);
}

int rrt_nystrom_output_batched_f32(const float* qkv, const float* kl, const float* wz, const float* conv_w, float* o, int64_t b,
                                   int64_t n_padded, int32_t heads, int32_t conv_k, void* stream) {
  if (!qkv || !kl || !wz || !o) return RRT_E_INVALID;
  int rc = check_np_heads(n_padded, heads);
  if (!rc) rc = check_nystrom_batch(b);
  if (rc) return rc;
  if (conv_w && (conv_k < 1 || conv_k % 2 == 0 || conv_k > 63)) return unsupported("nystrom: residual_conv_kernel must be odd and <= 63");
  return (int)launch_nystrom_output(qkv, kl, wz, conv_w, o, (long)n_padded, heads, conv_k, (hipStream_t)stream, (int)b);
}

// ---- ... the Nystrom ablations of RRTEncoder: the attention layers here, the rest of the forward is api.hip's (encoder_tail)
int rrt_encoder_nystrom_workspace_size(const rrt_encoder_desc* desc, const rrt_encoder_nystrom_desc* nys, int64_t n_tokens,
                                       size_t* bytes) {
  if (!bytes) return RRT_E_INVALID;
  rrt_grid g{};
  int rc = check_encoder_nystrom(desc, nys, n_tokens, &g);
  if (rc) return rc;
  size_t tail = 0;
  rc = encoder_tail_workspace_size(desc, n_tokens, &tail);
  if (rc) return rc;
  *bytes = carve_encoder_nystrom(desc, nys, n_tokens, g, tail, nullptr).bytes;
  return RRT_OK;
}

int rrt_encoder_nystrom_forward_f32(const rrt_encoder_desc* desc, const rrt_encoder_nystrom_desc* nys,
                                    const rrt_encoder_weights* w, const float* x, float* y, int64_t n_tokens, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  if (!desc || !nys || !w || !x || !y || x == y) return RRT_E_INVALID;
  rrt_grid g{};
  int rc = check_encoder_nystrom(desc, nys, n_tokens, &g);
  if (rc) return rc;
  size_t tail = 0;
  rc = encoder_tail_workspace_size(desc, n_tokens, &tail);
  if (rc) return rc;
  if (!workspace || workspace_bytes < carve_encoder_nystrom(desc, nys, n_tokens, g, tail, nullptr).bytes) return RRT_E_WORKSPACE;
  return encoder_nystrom_forward(desc, nys, w, x, y, n_tokens, g, carve_encoder_nystrom(desc, nys, n_tokens, g, tail, (char*)workspace),
                                 (hipStream_t)stream);
}

// ---- ... training: the stashing forward, the backward and its stages (nystrom_bwd.hip)
int rrt_nystrom_train_sizes(const rrt_nystrom_desc* desc, int64_t n, size_t* stash_bytes, size_t* backward_workspace_bytes) {
  if (!stash_bytes || !backward_workspace_bytes) return RRT_E_INVALID;
  int rc = check_nystrom(desc, n);
  if (rc) return rc;
  *stash_bytes = carve_nystrom_stash(desc, n, nullptr).bytes;
  *backward_workspace_bytes = carve_nystrom_bwd(desc, n, nullptr).bytes;
  return RRT_OK;
}

int rrt_nystrom_attention_forward_train_f32(const rrt_nystrom_desc* desc, const rrt_nystrom_weights* w, const float* x, float* y,
                                            int64_t n, void* stash, size_t stash_bytes, void* stream) {
  if (!desc || !w || !x || !y) return RRT_E_INVALID;
  int rc = check_nystrom(desc, n);
  if (rc) return rc;
  if (!nystrom_weights_ok(desc, w)) return RRT_E_INVALID;
  if (!stash || stash_bytes < carve_nystrom_stash(desc, n, nullptr).bytes) return RRT_E_WORKSPACE;
  const NystromStash s = carve_nystrom_stash(desc, n, (char*)stash);
  return nystrom_forward(desc, w, x, y, n, s.f, (hipStream_t)stream, s.lse);
}

int rrt_nystrom_attention_backward_f32(const rrt_nystrom_desc* desc, const rrt_nystrom_weights* w, const float* x,
                                       const float* dy, const void* stash, size_t stash_bytes, const rrt_nystrom_grads* grads,
                                       float* dx, int64_t n, void* workspace, size_t workspace_bytes, void* stream) {
  if (!desc || !w || !x || !dy || !grads) return RRT_E_INVALID;
  int rc = check_nystrom(desc, n);
  if (rc) return rc;
  if (!nystrom_weights_ok(desc, w)) return RRT_E_INVALID;
  if (!grads->qkv_w || !grads->out_w || !grads->out_b || (desc->residual && !grads->conv_w)) return RRT_E_INVALID;
  if (!stash || stash_bytes < carve_nystrom_stash(desc, n, nullptr).bytes) return RRT_E_WORKSPACE;
  if (!workspace || workspace_bytes < carve_nystrom_bwd(desc, n, nullptr).bytes) return RRT_E_WORKSPACE;
  return nystrom_backward(desc, w, x, dy, carve_nystrom_stash(desc, n, (char*)stash), carve_nystrom_bwd(desc, n, (char*)workspace),
                          grads, dx, n, (hipStream_t)stream);
}

int rrt_nystrom_output_backward_workspace_size(int64_t n_padded, int32_t heads, size_t* bytes) {
  if (!bytes) return RRT_E_INVALID;
  int rc = check_np_heads(n_padded, heads);
  if (rc) return rc;
  Arena a{nullptr};
  a.take(nystrom_output_bwd_floats((long)n_padded, heads));
  *bytes = a.bytes();
  return RRT_OK;
}

int rrt_nystrom_output_backward_f32(const float* qkv, const float* kl, const float* wz, const float* conv_w, const float* d_o,
                                    float* d_qkv, float* d_kl, float* d_wz, float* d_conv_w, int64_t n_padded, int32_t heads,
                                    int32_t conv_k, void* workspace, size_t workspace_bytes, void* stream) {
  if (!qkv || !kl || !wz || !d_o || !d_qkv || !d_kl || !d_wz || (conv_w && !d_conv_w)) return RRT_E_INVALID;
  int rc = check_np_heads(n_padded, heads);
  if (rc) return rc;
  if (conv_w && (conv_k < 1 || conv_k % 2 == 0 || conv_k > 63)) return unsupported("nystrom: residual_conv_kernel must be odd and <= 63");
  Arena a{(char*)workspace};
  float* part = a.take(nystrom_output_bwd_floats((long)n_padded, heads));
  if (!workspace || workspace_bytes < a.bytes()) return RRT_E_WORKSPACE;
  return (int)launch_nystrom_output_backward(qkv, kl, wz, conv_w, d_o, d_qkv, d_kl, d_wz, d_conv_w, part, (long)n_padded, heads,
                                             conv_k, (hipStream_t)stream);
}

int rrt_nystrom_zav_backward_f32(const float* z, const float* av, const float* d_wz, float* d_z, float* d_av, int32_t heads,
                                 void* stream) {
  if (!z || !av || !d_wz || !d_z || !d_av) return RRT_E_INVALID;
  int rc = check_nystrom_heads(heads);
  if (rc) return rc;
  return (int)launch_nystrom_zav_backward(z, av, d_wz, d_z, d_av, heads, (hipStream_t)stream);
}

int rrt_nystrom_landmark_attn_backward_workspace_size(int64_t n_padded, int32_t heads, size_t* bytes) {
  if (!bytes) return RRT_E_INVALID;
  int rc = check_np_heads(n_padded, heads);
  if (rc) return rc;
  *bytes = carve_lattn_bwd(n_padded, heads, nullptr).bytes;
  return RRT_OK;
}

int rrt_nystrom_landmark_attn_backward_f32(const float* qkv, const float* ql, const float* d_av, float* d_qkv, float* d_ql,
                                           int64_t n_padded, int32_t heads, void* workspace, size_t workspace_bytes,
                                           void* stream) {
  if (!qkv || !ql || !d_av || !d_qkv || !d_ql) return RRT_E_INVALID;
  int rc = check_np_heads(n_padded, heads);
  if (rc) return rc;
  if (!workspace || workspace_bytes < carve_lattn_bwd(n_padded, heads, nullptr).bytes) return RRT_E_WORKSPACE;
  const LattnBwdWs ws = carve_lattn_bwd(n_padded, heads, (char*)workspace);
  hipStream_t st = (hipStream_t)stream;
  RRT_TRY(launch_nystrom_lattn(qkv, ql, ws.av, ws.fwd, (long)n_padded, heads, st, ws.lse));
  return (int)launch_nystrom_lattn_backward(qkv, ql, ws.av, ws.lse, d_av, d_qkv, d_ql, ws.bwd, (long)n_padded, heads, st);
}

int rrt_nystrom_pinv_sim_backward_workspace_size(int32_t heads, int32_t iterations, size_t* bytes) {
  if (!bytes) return RRT_E_INVALID;
  int rc = check_nystrom_heads(heads);
  if (!rc) rc = check_pinv_iterations(iterations);
  if (rc) return rc;
  *bytes = carve_pinv_sim_bwd(heads, iterations, nullptr).bytes;
  return RRT_OK;
}

int rrt_nystrom_pinv_sim_backward_f32(const float* ql, const float* kl, const float* d_z, float* d_ql, float* d_kl,
                                      int32_t heads, int32_t iterations, void* workspace, size_t workspace_bytes, void* stream) {
  if (!ql || !kl || !d_z || !d_ql || !d_kl) return RRT_E_INVALID;
  int rc = check_nystrom_heads(heads);
  if (!rc) rc = check_pinv_iterations(iterations);
  if (rc) return rc;
  if (!workspace || workspace_bytes < carve_pinv_sim_bwd(heads, iterations, nullptr).bytes) return RRT_E_WORKSPACE;
  const PinvSimBwdWs ws = carve_pinv_sim_bwd(heads, iterations, (char*)workspace);
  hipStream_t st = (hipStream_t)stream;
  RRT_TRY(launch_nystrom_sim2(ql, kl, ws.a2, heads, st));
  return (int)launch_nystrom_pinv_sim_backward(ql, kl, ws.a2, d_z, d_ql, d_kl, 0, ws.bwd, heads, iterations, st);
}

int rrt_nystrom_landmarks_backward_f32(const float* d_ql, const float* d_kl, float* d_qkv, int64_t n_padded, int32_t heads,
                                       void* stream) {
  if (!d_ql || !d_kl || !d_qkv) return RRT_E_INVALID;
  int rc = check_np_heads(n_padded, heads);
  if (rc) return rc;
  return (int)launch_nystrom_landmarks_backward(d_ql, d_kl, d_qkv, (long)n_padded, heads, (hipStream_t)stream);
}

// ---- ... b sequences per launch, training (the b = 1 calls are the single-sequence ones, launch for launch)
int rrt_nystrom_batched_train_sizes(const rrt_nystrom_desc* desc, int64_t b, int64_t n, size_t* stash_bytes,
                                    size_t* backward_workspace_bytes) {
  if (!stash_bytes || !backward_workspace_bytes) return RRT_E_INVALID;
  int rc = check_nystrom_train_batched(desc, b, n);
  if (rc) return rc;
  *stash_bytes = carve_nystrom_stash(desc, n, nullptr, true, b).bytes;
  *backward_workspace_bytes = carve_nystrom_bwd(desc, n, nullptr, b).bytes;
  return RRT_OK;
}

int rrt_nystrom_attention_batched_forward_train_f32(const rrt_nystrom_desc* desc, const rrt_nystrom_weights* w, const float* x,
                                                    float* y, int64_t b, int64_t n, void* stash, size_t stash_bytes,
                                                    void* stream) {
  if (!desc || !w || !x || !y) return RRT_E_INVALID;
  int rc = check_nystrom_train_batched(desc, b, n);
  if (rc) return rc;
  if (!nystrom_weights_ok(desc, w)) return RRT_E_INVALID;
  if (!stash || stash_bytes < carve_nystrom_stash(desc, n, nullptr, true, b).bytes) return RRT_E_WORKSPACE;
  const NystromStash s = carve_nystrom_stash(desc, n, (char*)stash, true, b);
  hipStream_t st = (hipStream_t)stream;
  if (b == 1) return nystrom_forward(desc, w, x, y, n, s.f, st, s.lse);
  const float* o = nullptr;
  rc = nystrom_batched_front(desc, w, x, n, s.f, st, &o, s.lse);
  if (rc) return rc;
  LinearEpilogue eo{};
  eo.bias = w->out_b;
  RRT_TRY(launch_linear(o, w->out_w, y, (int)(b * n), desc->dim, desc->heads * 64, eo, st));
  return RRT_OK;
}

int rrt_nystrom_attention_batched_backward_f32(const rrt_nystrom_desc* desc, const rrt_nystrom_weights* w, const float* x,
                                               const float* dy, const void* stash, size_t stash_bytes,
                                               const rrt_nystrom_grads* grads, float* dx, int64_t b, int64_t n, void* workspace,
                                               size_t workspace_bytes, void* stream) {
  if (!desc || !w || !x || !dy || !grads) return RRT_E_INVALID;
  int rc = check_nystrom_train_batched(desc, b, n);
  if (rc) return rc;
  if (!nystrom_weights_ok(desc, w)) return RRT_E_INVALID;
  if (!grads->qkv_w || !grads->out_w || !grads->out_b || (desc->residual && !grads->conv_w)) return RRT_E_INVALID;
  if (!stash || stash_bytes < carve_nystrom_stash(desc, n, nullptr, true, b).bytes) return RRT_E_WORKSPACE;
  if (!workspace || workspace_bytes < carve_nystrom_bwd(desc, n, nullptr, b).bytes) return RRT_E_WORKSPACE;
  const NystromStash s = carve_nystrom_stash(desc, n, (char*)stash, true, b);
  const NystromBwdWs bw = carve_nystrom_bwd(desc, n, (char*)workspace, b);
  if (b == 1) return nystrom_backward(desc, w, x, dy, s, bw, grads, dx, n, (hipStream_t)stream);
  return nystrom_backward_batched(desc, w, x, dy, s, bw, grads, dx, n, (hipStream_t)stream);
}

int rrt_nystrom_output_batched_backward_workspace_size(int64_t b, int64_t n_padded, int32_t heads, size_t* bytes) {
  if (!bytes) return RRT_E_INVALID;
  int rc = check_stage_batched(b, n_padded, heads);
  if (rc) return rc;
  Arena a{nullptr};
  a.take(nystrom_output_bwd_floats((long)n_padded, heads, (int)b));
  *bytes = a.bytes();
  return RRT_OK;
}

int rrt_nystrom_output_batched_backward_f32(const float* qkv, const float* kl, const float* wz, const float* conv_w,
                                            const float* d_o, float* d_qkv, float* d_kl, float* d_wz, float* d_conv_w, int64_t b,
                                            int64_t n_padded, int32_t heads, int32_t conv_k, void* workspace,
                                            size_t workspace_bytes, void* stream) {
  if (!qkv || !kl || !wz || !d_o || !d_qkv || !d_kl || !d_wz || (conv_w && !d_conv_w)) return RRT_E_INVALID;
  int rc = check_stage_batched(b, n_padded, heads);
  if (rc) return rc;
  if (conv_w && (conv_k < 1 || conv_k % 2 == 0 || conv_k > 63)) return unsupported("nystrom: residual_conv_kernel must be odd and <= 63");
  Arena a{(char*)workspace};
  float* part = a.take(nystrom_output_bwd_floats((long)n_padded, heads, (int)b));
  if (!workspace || workspace_bytes < a.bytes()) return RRT_E_WORKSPACE;
  return (int)launch_nystrom_output_backward(qkv, kl, wz, conv_w, d_o, d_qkv, d_kl, d_wz, d_conv_w, part, (long)n_padded, heads,
                                             conv_k, (hipStream_t)stream, (int)b);
}

int rrt_nystrom_zav_batched_backward_f32(const float* z, const float* av, const float* d_wz, float* d_z, float* d_av, int64_t b,
                                         int32_t heads, void* stream) {
  if (!z || !av || !d_wz || !d_z || !d_av) return RRT_E_INVALID;
  int rc = check_stage_batched(b, heads);
  if (rc) return rc;
  return (int)launch_nystrom_zav_backward(z, av, d_wz, d_z, d_av, heads, (hipStream_t)stream, (int)b);
}

int rrt_nystrom_landmark_attn_batched_backward_workspace_size(int64_t b, int64_t n_padded, int32_t heads, size_t* bytes) {
  if (!bytes) return RRT_E_INVALID;
  int rc = check_stage_batched(b, n_padded, heads);
  if (rc) return rc;
  *bytes = carve_lattn_bwd(n_padded, heads, nullptr, (int)b).bytes;
  return RRT_OK;
}

int rrt_nystrom_landmark_attn_batched_backward_f32(const float* qkv, const float* ql, const float* d_av, float* d_qkv, float* d_ql,
                                                   int64_t b, int64_t n_padded, int32_t heads, void* workspace,
                                                   size_t workspace_bytes, void* stream) {
  if (!qkv || !ql || !d_av || !d_qkv || !d_ql) return RRT_E_INVALID;
  int rc = check_stage_batched(b, n_padded, heads);
  if (rc) return rc;
  if (!workspace || workspace_bytes < carve_lattn_bwd(n_padded, heads, nullptr, (int)b).bytes) return RRT_E_WORKSPACE;
  const LattnBwdWs ws = carve_lattn_bwd(n_padded, heads, (char*)workspace, (int)b);
  hipStream_t st = (hipStream_t)stream;
  RRT_TRY(launch_nystrom_lattn(qkv, ql, ws.av, ws.fwd, (long)n_padded, heads, st, ws.lse, (int)b));
  return (int)launch_nystrom_lattn_backward(qkv, ql, ws.av, ws.lse, d_av, d_qkv, d_ql, ws.bwd, (long)n_padded, heads, st, (int)b);
}

int rrt_nystrom_pinv_sim_batched_backward_workspace_size(int64_t b, int32_t heads, int32_t iterations, size_t* bytes) {
  if (!bytes) return RRT_E_INVALID;
  int rc = check_stage_batched(b, heads);
  if (!rc) rc = check_pinv_iterations(iterations);
  if (rc) return rc;
  *bytes = carve_pinv_sim_bwd(heads, iterations, nullptr, (int)b).bytes;
  return RRT_OK;
}

int rrt_nystrom_pinv_sim_batched_backward_f32(const float* ql, const float* kl, const float* d_z, float* d_ql, float* d_kl,
                                              int64_t b, int32_t heads, int32_t iterations, void* workspace,
                                              size_t workspace_bytes, void* stream) {
  if (!ql || !kl || !d_z || !d_ql || !d_kl) return RRT_E_INVALID;
  int rc = check_stage_batched(b, heads);
  if (!rc) rc = check_pinv_iterations(iterations);
  if (rc) return rc;
  if (!workspace || workspace_bytes < carve_pinv_sim_bwd(heads, iterations, nullptr, (int)b).bytes) return RRT_E_WORKSPACE;
  const PinvSimBwdWs ws = carve_pinv_sim_bwd(heads, iterations, (char*)workspace, (int)b);
  hipStream_t st = (hipStream_t)stream;
  RRT_TRY(launch_nystrom_sim2(ql, kl, ws.a2, heads, st, (int)b));
  return (int)launch_nystrom_pinv_sim_backward(ql, kl, ws.a2, d_z, d_ql, d_kl, 0, ws.bwd, heads, iterations, st, (int)b);
}

int rrt_nystrom_landmarks_batched_backward_f32(const float* d_ql, const float* d_kl, float* d_qkv, int64_t b, int64_t n_padded,
                                               int32_t heads, void* stream) {
  if (!d_ql || !d_kl || !d_qkv) return RRT_E_INVALID;
  int rc = check_stage_batched(b, n_padded, heads);
  if (rc) return rc;
  return (int)launch_nystrom_landmarks_backward(d_ql, d_kl, d_qkv, (long)n_padded, heads, (hipStream_t)stream, (int)b);
}

int rrt_nystrom_output_row_f32(const float* qkv, const float* kl, const float* wz, const float* conv_w, float* o_row, int64_t row,
                               int64_t n_padded, int32_t heads, int32_t conv_k, void* stream) {
  if (!qkv || !kl || !wz || !o_row) return RRT_E_INVALID;
  int rc = check_output_row(row, n_padded, heads, conv_w, conv_k);
  if (rc) return rc;
  return (int)launch_nystrom_output_row(qkv, kl, wz, conv_w, o_row, (long)row, (long)n_padded, heads, conv_k, (hipStream_t)stream);
}

int rrt_nystrom_output_row_backward_f32(const float* qkv, const float* kl, const float* wz, const float* conv_w,
                                        const float* d_o_row, float* d_qkv, float* d_kl, float* d_wz, float* d_conv_w, int64_t row,
                                        int64_t n_padded, int32_t heads, int32_t conv_k, void* stream) {
  if (!qkv || !kl || !wz || !d_o_row || !d_qkv || !d_kl || !d_wz || (conv_w && !d_conv_w)) return RRT_E_INVALID;
  int rc = check_output_row(row, n_padded, heads, conv_w, conv_k);
  if (rc) return rc;
  return (int)launch_nystrom_output_row_backward(qkv, kl, wz, conv_w, d_o_row, d_qkv, d_kl, d_wz, d_conv_w, (long)row,
                                                 (long)n_padded, heads, conv_k, (hipStream_t)stream);
}

// ---- TransMIL: PPEG on the square part of the sequence, the forward, the forward with attention maps
int rrt_ppeg_side_f32(const float* x, const float* const* w, const float* const* b, float* y, int32_t side, int32_t dim,
                      void* stream) {
  if (!x || !y || !w || !w[0] || !w[1] || !w[2] || side <= 0 || dim <= 0) return RRT_E_INVALID;
  if (dim % 4) return unsupported("ppeg: dim must be a multiple of 4");
  if (side > 1000) return unsupported("ppeg: side above 1000");
  const float* nob[3] = {nullptr, nullptr, nullptr};
  hipStream_t st = (hipStream_t)stream;
  RRT_TRY(hipMemcpyAsync(y, x, (size_t)dim * sizeof(float), hipMemcpyDeviceToDevice, st));
  return (int)launch_ppeg_side(x + dim, w, b ? b : nob, y + dim, side, dim, st);
}

int rrt_transmil_workspace_size(const rrt_transmil_desc* desc, int64_t n_tokens, size_t* bytes) {
  if (!bytes) return RRT_E_INVALID;
  int rc = check_transmil(desc, n_tokens);
  if (rc) return rc;
  *bytes = carve_transmil(desc, n_tokens, nullptr).bytes;
  return RRT_OK;
}

int rrt_transmil_forward_f32(const rrt_transmil_desc* desc, const rrt_transmil_weights* w, const float* x, float* logits,
                             float* feat, int64_t n_tokens, void* workspace, size_t workspace_bytes, void* stream) {
  if (!desc || !w || !x || !logits) return RRT_E_INVALID;
  int rc = check_transmil(desc, n_tokens);
  if (rc) return rc;
  if (!transmil_weights_ok(desc, w)) return RRT_E_INVALID;
  if (!workspace || workspace_bytes < carve_transmil(desc, n_tokens, nullptr).bytes) return RRT_E_WORKSPACE;
  return transmil_forward(desc, w, x, logits, feat, nullptr, nullptr, n_tokens, carve_transmil(desc, n_tokens, (char*)workspace),
                          RowWs{}, (hipStream_t)stream);
}

int rrt_transmil_attn_workspace_size(const rrt_transmil_desc* desc, int64_t n_tokens, size_t* bytes) {
  if (!bytes) return RRT_E_INVALID;
  int rc = check_transmil(desc, n_tokens);
  if (rc) return rc;
  *bytes = carve_row(carve_transmil(desc, n_tokens, nullptr).bytes, desc->attn.heads, nullptr).bytes;
  return RRT_OK;
}

int rrt_transmil_forward_attn_f32(const rrt_transmil_desc* desc, const rrt_transmil_weights* w, const float* x, float* logits,
                                  float* feat, float* attn1, float* attn2, int64_t n_tokens, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  if (!desc || !w || !x || !logits) return RRT_E_INVALID;
  int rc = check_transmil(desc, n_tokens);
  if (rc) return rc;
  if (!transmil_weights_ok(desc, w)) return RRT_E_INVALID;
  const size_t front = carve_transmil(desc, n_tokens, nullptr).bytes;
  if (!workspace || workspace_bytes < carve_row(front, desc->attn.heads, nullptr).bytes) return RRT_E_WORKSPACE;
  return transmil_forward(desc, w, x, logits, feat, attn1, attn2, n_tokens, carve_transmil(desc, n_tokens, (char*)workspace),
                          carve_row(front, desc->attn.heads, (char*)workspace), (hipStream_t)stream);
}

// ---- ... the one-call training step, its cls-row twins and the stages only the step has
int rrt_transmil_train_sizes(const rrt_transmil_desc* desc, int64_t n_tokens, size_t* stash_bytes, size_t* backward_workspace_bytes) {
  return transmil_train_sizes(desc, n_tokens, stash_bytes, backward_workspace_bytes, false);
}

int rrt_transmil_forward_train_f32(const rrt_transmil_desc* desc, const rrt_transmil_weights* w, const float* x, float* logits,
                                   int64_t n_tokens, void* stash, size_t stash_bytes, float fc1_drop_p, float attn_drop_p,
                                   uint64_t drop_seed, void* stream) {
  return transmil_forward_train_entry(desc, w, x, logits, n_tokens, stash, stash_bytes, fc1_drop_p, attn_drop_p, drop_seed, stream,
                                      false);
}

int rrt_transmil_backward_f32(const rrt_transmil_desc* desc, const rrt_transmil_weights* w, const float* x, const float* d_logits,
                              const void* stash, size_t stash_bytes, const rrt_transmil_grads* grads, float* dx, int64_t n_tokens,
                              void* workspace, size_t workspace_bytes, float fc1_drop_p, float attn_drop_p, uint64_t drop_seed,
                              void* stream) {
  return transmil_backward_entry(desc, w, x, d_logits, stash, stash_bytes, grads, dx, n_tokens, workspace, workspace_bytes,
                                 fc1_drop_p, attn_drop_p, drop_seed, stream, false);
}

int rrt_debug_transmil_train_sizes_row(const rrt_transmil_desc* desc, int64_t n_tokens, size_t* stash_bytes,
                                        size_t* backward_workspace_bytes) {
  return transmil_train_sizes(desc, n_tokens, stash_bytes, backward_workspace_bytes, true);
}

int rrt_debug_transmil_forward_train_row_f32(const rrt_transmil_desc* desc, const rrt_transmil_weights* w, const float* x,
                                              float* logits, int64_t n_tokens, void* stash, size_t stash_bytes, float fc1_drop_p,
                                              float attn_drop_p, uint64_t drop_seed, void* stream) {
  return transmil_forward_train_entry(desc, w, x, logits, n_tokens, stash, stash_bytes, fc1_drop_p, attn_drop_p, drop_seed, stream,
                                      true);
}

int rrt_debug_transmil_backward_row_f32(const rrt_transmil_desc* desc, const rrt_transmil_weights* w, const float* x,
                                         const float* d_logits, const void* stash, size_t stash_bytes,
                                         const rrt_transmil_grads* grads, float* dx, int64_t n_tokens, void* workspace,
                                         size_t workspace_bytes, float fc1_drop_p, float attn_drop_p, uint64_t drop_seed,
                                         void* stream) {
  return transmil_backward_entry(desc, w, x, d_logits, stash, stash_bytes, grads, dx, n_tokens, workspace, workspace_bytes,
                                 fc1_drop_p, attn_drop_p, drop_seed, stream, true);
}

int rrt_ppeg_side_backward_workspace_size(int32_t side, int32_t dim, size_t* bytes) {
  if (!bytes || side <= 0 || dim <= 0) return RRT_E_INVALID;
  if (dim % 4) return unsupported("ppeg: dim must be a multiple of 4");
  if (side > 1000) return unsupported("ppeg: side above 1000");
  *bytes = ppeg_side_bwd_workspace(side, dim);
  return RRT_OK;
}

int rrt_ppeg_side_backward_f32(const float* x, const float* dy, const float* const* w, float* dx, float* const* dw,
                               float* const* db, int32_t side, int32_t dim, void* workspace, size_t workspace_bytes, void* stream) {
  if (!x || !dy || !dx || !w || !w[0] || !w[1] || !w[2] || !dw || !dw[0] || !dw[1] || !dw[2] || side <= 0 || dim <= 0)
    return RRT_E_INVALID;
  if (dim % 4) return unsupported("ppeg: dim must be a multiple of 4");
  if (side > 1000) return unsupported("ppeg: side above 1000");
  if (!workspace || workspace_bytes < ppeg_side_bwd_workspace(side, dim)) return RRT_E_WORKSPACE;
  float* const nob[3] = {nullptr, nullptr, nullptr};
  return (int)launch_ppeg_side_backward(x, dy, w, dx, dw, db ? db : nob, side, dim, workspace, (hipStream_t)stream);
}

int rrt_transmil_assemble_backward_f32(const float* d_seq, const float* hpre, float* d_emb, float* d_cls, int64_t n_tokens,
                                       int32_t dim, int32_t act, float drop_p, uint64_t drop_seed, void* stream) {
  if (!d_seq || !d_emb || !d_cls || n_tokens <= 0 || dim <= 0) return RRT_E_INVALID;
  if (n_tokens > 998001) return unsupported("transmil: n_tokens above 998001");
  if (dim % 4) return unsupported("transmil: dim must be a multiple of 4");
  if (act != RRT_ACT_NONE && act != RRT_ACT_RELU && act != RRT_ACT_GELU) return unsupported("transmil: act must be none/relu/gelu");
  if (act != RRT_ACT_NONE && !hpre) return RRT_E_INVALID;
  DropCfg dc{};
  if (make_drop(drop_p, &dc)) return RRT_E_INVALID;
  return (int)launch_transmil_assemble_backward(d_seq, hpre, d_emb, d_cls, (int)n_tokens, ceil_sqrt_i64(n_tokens), dim, act,
                                                dc.thresh, dc.seed(drop_seed, DROP_TAG_FC1), dc.scale, (hipStream_t)stream);
}
}  // extern "C"
