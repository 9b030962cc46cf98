// api_internal.h -- what the host-only units behind include/rrt_hip.h (api.hip, api_nystrom.hip) share: the workspace bump
// allocator, the HIP-error early return, and the declarations of the helpers of api.hip that api_nystrom.hip calls.  Each is
// defined once; everything else of a unit stays in that unit's anonymous namespace.
#pragma once
#include "internal.h"

// a failed launch (or any other HIP call) ends the entry point with the HIP error as its return code
#define RRT_TRY(call)                     \
  do {                                    \
    const hipError_t e_ = (call);         \
    if (e_ != hipSuccess) return (int)e_; \
  } while (0)

namespace rrt_api {
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// The one bump allocator behind every workspace carve.  A carve function states its layout once, as a sequence of take()s,
// and serves both the size query (base = null: every pointer is null, only bytes() counts) and the real carve, so a size can
// never disagree with the pointers handed out.  Every piece starts on a 256-byte boundary.
struct Arena {
  char* base;
  size_t off = 0;
  template <typename T = float>
  T* take(size_t count) {
    T* p = base ? (T*)(base + off) : nullptr;
    off = align_up(off + count * sizeof(T), 256);
    return p;
  }
  size_t bytes() const { return off; }
};

// RRT_E_UNSUPPORTED with `why` as the calling thread's detail string, which rrt_strerror reports (defined in api.hip, beside
// the string itself)
int unsupported(const char* why);

// dropout of one training call -- keep threshold and rescale; seed(): one layer's mask word (tests/hip_util.py)
struct DropCfg {
  unsigned thresh;
  float scale;
  unsigned seed(uint64_t base, int layer) const { return (unsigned)(base ^ (base >> 32)) + 0x9E3779B9u * (unsigned)(layer + 1); }
};
// fills it from a probability; RRT_E_INVALID outside [0, 1) (defined in api.hip, beside unsupported)
int make_drop(float p, DropCfg* d);

// The part of an encoder forward behind its attention layers -- CR-MSA, all_shortcut, the final LayerNorm -- exactly as
// rrt_encoder_forward_f32 runs it on a descriptor with n_rmsa_layers = 0 and pos = none: x1 [n_tokens, dim] the layers' result,
// x0 what all_shortcut adds (the forward's original input), workspace of encoder_tail_workspace_size bytes (defined in api.hip)
int encoder_tail_workspace_size(const rrt_encoder_desc* desc, int64_t n_tokens, size_t* bytes);
int encoder_tail(const rrt_encoder_desc* desc, const rrt_encoder_weights* w, const float* x1, const float* x0, float* y,
                 int64_t n_tokens, void* workspace, size_t workspace_bytes, void* stream);

// ---- the front every head around the encoder shares, and the ABMIL tail (defined in api.hip, where their comments are)
struct HeadFront {
  const rrt_encoder_desc* enc;   // (enc->dim is the embedding width whether or not there is an encoder)
  int input_dim, emb_act, has_rrt;
  int input16;                   // RRTMIL: the caller's features ARE the 16-bit operand (RRT_COMPUTE_BF16 / F16), else 0
};
struct HeadWs {
  float *emb, *y;      // (y == emb without an encoder)
  char *enc_ws, *head;
  size_t enc_bytes;
  uint16_t *x16, *w16, *y16, *pa16, *pb16;
  size_t bytes;
};
struct PoolWs {
  float *hid_a, *hid_b, *a_raw, *part;
  size_t bytes;
};
int gemm_precision(int compute);
int check_head_front(const HeadFront& f, int64_t N);
int carve_head(const HeadFront& f, int64_t N, size_t head_bytes, int pool16_hidden, char* base, HeadWs* out);
int head_front_forward(const HeadFront& f, const HeadWs& ws, const float* x, const float* emb_w, const float* emb_b,
                       const rrt_encoder_weights* enc_w, const float* pool_a_w, const float* pool_b_w, int pool_hidden,
                       float* y_out, bool tuning, int64_t N, void* stream, bool* p16);
PoolWs carve_pool(int64_t N, int dim, int hidden, int gated, char* base);
int check_pool(int64_t N, int dim, int hidden, int act, int n_classes);
int pool_predict(const float* y, const float* a_w, const float* a_b, const float* b_w, const float* b_b, const float* c_w,
                 const float* c_b, const float* pred_w, const float* pred_b, float* pooled, float* logits, float* attn,
                 int no_norm, int64_t N, int dim, int hidden, int act, int n_classes, int compute, const PoolWs& ws,
                 hipStream_t st, const uint16_t* y16 = nullptr, const uint16_t* a_w16 = nullptr,
                 const uint16_t* b_w16 = nullptr);
}  // namespace rrt_api
