// Host-side Q-network: the precision-independent model object (model.hip), the model_* functions the learner composes,
// and the two backends they choose between (bf16: qnet_bf16.hip, fp32: qnet32.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "profiler.h"
#include "qlx_internal.h"

namespace qlx {

constexpr int kNumVars = 10;
constexpr int64_t kVarOffsetDense = 77984;   // flat offset of W3 (conv variables before it, dense ones after)
constexpr int64_t kNumParams = 1685667;   // sum of the 10 Keras variables (variables.index shapes)
extern const int kVarSize[kNumVars];
inline int64_t var_offset(int v) {   // flat offset of variable v in d_params / d_m / d_v / d_grads
  int64_t o = 0;
  for (int i = 0; i < v; ++i) o += kVarSize[i];
  return o;
}
inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

constexpr int kF32FwdChunk = 8192;   // samples per fp32 forward pass (bounds the a1..a3 workspace)

// Carves one allocation into 256-byte-aligned buffers.  A layout runs twice: from base 0 for the size, then from the
// allocation for the pointers.
struct Arena {
  uintptr_t base = 0;
  size_t off = 0;
  template <class T>
  T* take(size_t count) {
    T* p = reinterpret_cast<T*>(base + off);
    off = align_up(off + count * sizeof(T), 256);
    return p;
  }
};

struct CommonWs {   // the per-batch buffers both backends use (the head's inputs and outputs are fp32 in either)
  uint8_t* frames = nullptr;          // [B*4][7056] s2d staging for host observations
  const uint8_t** table = nullptr;    // [B][4] frame pointers
  float* q = nullptr;
  float *gs = nullptr, *hs = nullptr, *y = nullptr, *rew = nullptr;
  uint8_t *act = nullptr, *argmax = nullptr, *done = nullptr;
  float* loss = nullptr;
};

struct Bf16Net;   // qnet_bf16.hip
struct F32Net;    // qnet32.hip

}  // namespace qlx

struct qlx_head;   // head_wide.hip

struct qlx_model {
  int device = 0;
  bool f32 = true;   // QLX_ARCH_NATURE_DQN: fp32 (the reference's arithmetic); QLX_ARCH_NATURE_DQN_BF16: bf16 MFMA operands
  hipStream_t stream = nullptr;
  bool own_stream = true;
  qlx::DeviceBuffer<float> d_params;   // fp32 master weights, Keras layouts, variables concatenated
  qlx::DeviceBuffer<float> d_m, d_v, d_grads, d_norms;
  int64_t iterations = 0;
  uint64_t version = 0;   // bumped by model_pack, i.e. on every write of the weights from outside the optimizer
  float lr = 0.00025f, beta1 = 0.9f, beta2 = 0.999f, eps = 1e-7f, clipnorm = 1.0f;
  qlx::DeviceBuffer<uint8_t> ws;   // one allocation: the common buffers (w), then the backend's
  int ws_batch = 0;
  int last_batch = 0;
  // The last trunk forward (model_forward_trunk), for qlx_model_backward_dev: its ticket (a counter, never 0), the table it
  // read, and whether a backward may still use what it left - it stored its activations, and neither the weights
  // (model_adam, model_pack) nor the workspace changed since.  grads_filled: a backward (or qlx_model_apply_gradient) has
  // written d_grads.
  uint64_t fwd_ticket = 1;
  const uint8_t* const* fwd_table = nullptr;
  bool fwd_reusable = false;
  bool grads_filled = false;
  // the attached wide head (head_wide.hip; at most one, fp32 models only) and whether the gradient now in the buffers came
  // from qlx_head_backward_dev: only then does qlx_model_step_dev step the head as well (every other backward clears it)
  qlx_head* head = nullptr;
  bool head_grads = false;
  qlx::CommonWs w;
  qlx::Profiler* prof = nullptr;   // set by the learner while profiling
  // the _dev calls (model_dev.hip), all set by qlx_model_reserve: the largest n they may run, the sticky flag word
  // (bit 0 an index >= len, bit 1 an action >= 3), the checked copy of the caller's actions and the max-Q head's zero
  // rewards / dones; the event orders qlx_model_copy_weights_dev across two streams (created at its first use)
  uint32_t dev_reserved = 0;
  qlx::DeviceBuffer<uint32_t> d_dev_flag;
  qlx::DeviceBuffer<uint8_t> d_dev_act;
  qlx::DeviceBuffer<float> d_dev_zero;
  hipEvent_t dev_event = nullptr;
  // the backend's own state (operand copies, activations, norm partials, update-tail flags): exactly one is set, and
  // only that backend's file sees inside it
  qlx::Bf16Net* bf16 = nullptr;
  qlx::F32Net* fp32 = nullptr;
};

namespace qlx {
struct Fc2Args {
  const __bf16* a4;          // [B][512]
  const float* a4f;          // fp32 model: [B][512]
  // pending split-K fc1 partials (splits > 0): the head finishes a4 = relu(sum_z slab[z] + b3) in fixed z order
  // and writes it to a4_out, so no separate reduction launch runs
  const float* slab;
  size_t zstride;
  int splits;
  const float* b3;
  __bf16* a4_out;
  const float* w4;         // [512][3] master
  const float* b4;         // [3]
  int B;
  float* q;                // [B][3] out (may be null)
  uint8_t* argmax;         // mode 1
  const float* rewards;    // mode 2
  const uint8_t* dones;    // mode 2
  float gamma;             // mode 2
  float* y_out;            // mode 2
  const float* q_select;   // mode 2, double DQN: [B][3] online Q(s'), a* = its first argmax, y uses q[a*] (else max)
  const uint8_t* actions;  // training head
  const float* y;          // training head
  float* gsample;          // training head: dloss/dq_a per sample
  float* hsample;          // training head: per-sample Huber value
  const float* weights;    // training head (optional): per-sample loss weights (prioritized-replay IS weights)
  float* td_abs;           // training head (optional): |q_a - y| out
  float* dz4_out;          // fp32 training head (optional): the dense-3 backward dz4 [B][512], fused
};

// ---- the model layer (model.hip): each call is the backend's of the same name ----
void model_workspace(qlx_model* m, int B);
void model_pack(qlx_model* m);
// a sample's result must not depend on the batch it is evaluated in (the learner's target net, whose memo and per-batch
// pass evaluate the same transition at different batch sizes)
void model_set_batch_invariant(qlx_model* m);
// store_acts = false skips writing a1/a2 (only a3 is needed when no backward pass follows)
void model_forward_trunk(qlx_model* m, const uint8_t* const* table, int B, hipStream_t s, bool store_acts = true);
// head arguments for the model's last forward (bf16: consumes pending fc1 partials, the head launch that follows
// materialises a4), and the head launch: mode 0 q, 1 + argmax, 2 Bellman target
Fc2Args fc2_args(qlx_model* m, int B);
void model_head(qlx_model* m, int mode, const Fc2Args& a, int B, hipStream_t s);
// Huber head + backward after model_forward_trunk: loss -> *loss_dev, raw gradients -> m->d_grads
// weights (optional): per-sample loss weights; td_abs (optional): |q_a - y| per sample out.
// = model_backward_dense (head, fc1: the dense gradients, 95 % of the bytes, are final after it) followed by
// model_backward_conv (the conv trunk); a data-parallel caller all-reduces the dense bucket in between
// fuse_update: no all-reduce will follow, so the fp32 path may schedule the norms / Adam of the variables whose gradient
// is final inside the later backward launches (model_norms / model_adam then finish the rest)
void model_backward(qlx_model* m, const uint8_t* const* table, int B, const uint8_t* actions, const float* y, float* loss_dev,
                    hipStream_t s, const float* weights = nullptr, float* td_abs = nullptr, bool fuse_update = false);
void model_backward_dense(qlx_model* m, int B, const uint8_t* actions, const float* y, float* loss_dev, hipStream_t s,
                          const float* weights = nullptr, float* td_abs = nullptr);
// The backward of sum_{b,n} dq[b][n] Q[b][n] for a caller's dq [B][3] (device) in place of the Huber head, after
// model_forward_trunk on the same batch: raw gradients -> m->d_grads.  = model_backward_dq_dense (the dq head, fc1 and the
// dense-3 gradients; no loss) followed by model_backward_conv as it is.  A dq row that is 0 except at one action gives
// model_backward's gradients value for value.
void model_backward_dq(qlx_model* m, const uint8_t* const* table, int B, const float* dq, hipStream_t s, bool fuse_update = false);
void model_backward_dq_dense(qlx_model* m, int B, const float* dq, hipStream_t s);
// dense_ready (data parallel): the dense bucket's all-reduce event; the fp32 reduction launch then waits for it and computes
// the dense variables' clip-norm partials of the reduced gradient x dense_scale as its extra blocks (bf16 ignores both)
void model_backward_conv(qlx_model* m, const uint8_t* const* table, int B, hipStream_t s, bool fuse_update = false,
                         hipEvent_t dense_ready = nullptr, float dense_scale = 1.0f);
// The update tail.  Each backend keeps clip-norm partials its backward produced and knows whether they still belong to
// d_grads; a caller that writes d_grads itself says so with model_gradient_replaced (an all-reduce in place needs no
// call: the scale it passes tells).  model_norms_dense: the dense variables' partials of d_grads x scale, which may run as
// soon as the dense bucket is final (fp32; bf16 has no such split).  model_norms: whatever is still missing before
// model_adam at that scale.
void model_gradient_replaced(qlx_model* m);
void model_norms_dense(qlx_model* m, hipStream_t s, float scale);
void model_norms(qlx_model* m, hipStream_t s, float scale);
void model_adam(qlx_model* m, hipStream_t s, float scale);

// weights, Adam m and v ([3][kNumParams]) and the iteration count to / from host arrays (snapshots); put restores like a
// checkpoint read: the operand copies are rebuilt from the masters (model_pack) and the stream is synchronised
void model_state_get(qlx_model* m, float* out3, int64_t* iterations);
void model_state_put(qlx_model* m, const float* in3, int64_t iterations);

// the state-source checks and the frame table of the _dev calls (model_dev.hip), shared with the wide head's entry points
void check_source(const qlx_states_dev* s);
void check_handles(const qlx_model* m, const qlx_states_dev& s, uint32_t n);
const uint8_t* const* states_table(qlx_model* m, const qlx_states_dev& s, uint32_t n);
// clip_by_norm + Adam of the attached head on its own gradient buffer, its iterations + 1 (head_wide.hip)
void head_step(qlx_head* h, hipStream_t s);

// (Re)allocates m->ws for B samples: the common buffers, then whatever `layout` takes from the arena for the backend
void ws_common(qlx_model* m, Arena& a, int B);
template <class Layout>
void ws_alloc(qlx_model* m, int B, Layout&& layout) {
  QLX_HIP(hipStreamSynchronize(m->stream));
  m->ws.release();
  m->ws_batch = 0;
  Arena size;
  ws_common(m, size, B);
  layout(size);
  m->ws.alloc(size.off);
  Arena a{(uintptr_t)m->ws.get()};
  ws_common(m, a, B);
  layout(a);
  m->ws_batch = B;
}
// head arguments both backends fill alike
inline Fc2Args fc2_common(qlx_model* m, int B) {
  Fc2Args a{};
  a.w4 = m->d_params + var_offset(8);
  a.b4 = m->d_params + var_offset(9);
  a.b3 = m->d_params + var_offset(7);
  a.B = B;
  a.q = m->w.q;
  a.zstride = (size_t)B * 512;
  return a;
}

// ---- the backends: bf16_* (qnet_bf16.hip) and f32_* (qnet32.hip), chosen between by the model_* functions ----
void bf16_create(qlx_model* m);    // the backend's device state (m->bf16 / m->fp32), nothing of the common model
void bf16_destroy(qlx_model* m);
void bf16_workspace(qlx_model* m, int B);   // B > m->ws_batch
void bf16_pack(qlx_model* m);
void bf16_set_batch_invariant(qlx_model* m);
void bf16_forward(qlx_model* m, const uint8_t* const* table, int B, hipStream_t s, bool store_acts);
Fc2Args bf16_fc2_args(qlx_model* m, int B);
void bf16_head(int mode, const Fc2Args& a, int B, hipStream_t s);
void bf16_backward_dense(qlx_model* m, int B, const uint8_t* actions, const float* y, float* loss_dev, hipStream_t s,
                         const float* weights, float* td_abs);
void bf16_backward_dense_dq(qlx_model* m, int B, const float* dq, hipStream_t s);
void bf16_backward_conv(qlx_model* m, const uint8_t* const* table, int B, hipStream_t s);
void bf16_gradient_replaced(qlx_model* m);
void bf16_norms(qlx_model* m, hipStream_t s, float scale);
void bf16_adam(qlx_model* m, hipStream_t s, float scale);
void bf16_last_activation(qlx_model* m, int layer, float* out);

void f32_create(qlx_model* m);
void f32_destroy(qlx_model* m);
void f32_workspace(qlx_model* m, int B);
void f32_forward(qlx_model* m, const uint8_t* const* table, int B, hipStream_t s);
Fc2Args f32_fc2_args(qlx_model* m, int B);
void f32_head(int mode, const Fc2Args& a, int B, hipStream_t s);   // mode 3 = training head
void f32_backward_dense(qlx_model* m, int B, const uint8_t* actions, const float* y, float* loss_dev, hipStream_t s,
                        const float* weights, float* td_abs);
void f32_backward_dense_dq(qlx_model* m, int B, const float* dq, hipStream_t s);
void f32_backward_conv(qlx_model* m, const uint8_t* const* table, int B, hipStream_t s, bool fuse_update,
                       hipEvent_t dense_ready = nullptr, float dense_scale = 1.0f);
void f32_gradient_replaced(qlx_model* m);
void f32_norms(qlx_model* m, hipStream_t s, float scale);
void f32_adam(qlx_model* m, hipStream_t s, float scale);
void f32_last_activation(qlx_model* m, int layer, float* out);
// the wide head's backward (head_wide.hip) in place of k_head32_dq: a4 of the last forward; the dz4 buffer of a backward
// over B samples (the checks and the gradient workspace of f32_backward_dense_dq); then the fc1 backward with SideFc2Dq
// on the dz4 the caller wrote there
const float* f32_a4(qlx_model* m);
float* f32_dz4_begin(qlx_model* m, int B);
void f32_backward_dense_dz4(qlx_model* m, int B, const float* dq, hipStream_t s);
// fractions of a batch's fp32 conv work the exact skips leave out (qnet32.hip k_frame_sparsity; synchronises s):
// out = {conv1 forward zero steps, conv1 weight-gradient zero steps, conv2 background rows, conv3 background rows}
// d_cnt: 4 device counters, h_cnt: their pinned host copy (both the caller's, allocated once)
void frame_sparsity(const uint8_t* const* table, int n, unsigned long long* d_cnt, unsigned long long* h_cnt, double* out,
                    hipStream_t s);
}  // namespace qlx
