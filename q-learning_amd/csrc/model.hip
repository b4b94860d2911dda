// DeepQLearningModel, the part that does not depend on the arithmetic: the model object (master weights, Adam slots,
// gradient, workspace), initialisation, variables, checkpoints, the TF bundle loader, host-frame staging, the C ABI of
// qlx_model_*, and the model_* functions the learner composes - each the choice between the bf16 backend
// (qnet_bf16.hip) and the fp32 backend (qnet32.hip).  This is the only file that asks a model for its precision.
//
// Reference (restated): create_ql_model_breakout_84x84x4_3_32.py:20-33 (graph), :36-55 (predict_action,
// batch_predict_max_future_reward), :63-82 (train_model).  The reference runs this inside libtensorflow behind
// Session::run (q_learning_model.rs:107-189).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "objects.h"
#include "qnet.h"

namespace qlx {

const int kVarSize[kNumVars] = {8 * 8 * 4 * 32, 32, 4 * 4 * 32 * 64, 64, 3 * 3 * 64 * 64, 64, 3136 * 512, 512, 512 * 3, 3};

static_assert(8 * 8 * 4 * 32 + 32 + 4 * 4 * 32 * 64 + 64 + 3 * 3 * 64 * 64 + 64 == kVarOffsetDense, "dense bucket offset");

// ------------------------------------------------------------------------------------------
// host obs [B][x][y][slot] -> s2d frames [B*4][7056] + frame pointer table

__global__ void k_pack_obs(const uint8_t* obs, int B, uint8_t* frames) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // over B*84*84
  if (i >= (int64_t)B * kFramePix) return;
  const int b = (int)(i / kFramePix), xy = (int)(i - (int64_t)b * kFramePix);
  const int x = xy / kFrame, y = xy - x * kFrame;
  const uchar4 v = reinterpret_cast<const uchar4*>(obs)[i];
  const int off = s2d_offset(x, y);
  frames[((size_t)b * 4 + 0) * kFramePix + off] = v.x;
  frames[((size_t)b * 4 + 1) * kFramePix + off] = v.y;
  frames[((size_t)b * 4 + 2) * kFramePix + off] = v.z;
  frames[((size_t)b * 4 + 3) * kFramePix + off] = v.w;
}

__global__ void k_frame_table(const uint8_t* frames, int B, const uint8_t** table) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B * 4) table[i] = frames + (size_t)i * kFramePix;
}

// ------------------------------------------------------------------------------------------
// the model layer

void ws_common(qlx_model* m, Arena& a, int B) {
  CommonWs& w = m->w;
  w.frames = a.take<uint8_t>((size_t)B * 4 * kFramePix);
  w.table = a.take<const uint8_t*>((size_t)B * 4);
  w.q = a.take<float>((size_t)B * 3);
  w.gs = a.take<float>(B); w.hs = a.take<float>(B); w.y = a.take<float>(B);
  w.act = a.take<uint8_t>(B); w.argmax = a.take<uint8_t>(B); w.rew = a.take<float>(B); w.done = a.take<uint8_t>(B);
  w.loss = a.take<float>(16);
}

void model_workspace(qlx_model* m, int B) {
  if (B <= m->ws_batch) return;
  m->fwd_reusable = false;   // the activations go with the old allocation
  m->f32 ? f32_workspace(m, B) : bf16_workspace(m, B);
}

void model_pack(qlx_model* m) {
  m->version += 1;
  m->fwd_reusable = false;
  if (!m->f32) bf16_pack(m);   // the fp32 path reads the master weights directly
}

void model_set_batch_invariant(qlx_model* m) {
  if (!m->f32) bf16_set_batch_invariant(m);   // the fp32 kernels never depend on the batch size
}

void model_forward_trunk(qlx_model* m, const uint8_t* const* table, int B, hipStream_t s, bool store_acts) {
  if (++m->fwd_ticket == 0) m->fwd_ticket = 1;
  m->fwd_table = table;
  m->fwd_reusable = m->f32 || store_acts;   // (the fp32 forward always stores a1 .. a3)
  m->f32 ? f32_forward(m, table, B, s) : bf16_forward(m, table, B, s, store_acts);
}

Fc2Args fc2_args(qlx_model* m, int B) { return m->f32 ? f32_fc2_args(m, B) : bf16_fc2_args(m, B); }

void model_head(qlx_model* m, int mode, const Fc2Args& a, int B, hipStream_t s) {
  m->f32 ? f32_head(mode, a, B, s) : bf16_head(mode, a, B, s);
}

// Huber loss (mean over the batch -> *loss_dev) and its raw, unclipped gradients into m->d_grads, after
// model_forward_trunk on the same batch; actions / y are device arrays [B]
void model_backward(qlx_model* m, const uint8_t* const* table, int B, const uint8_t* actions, const float* y, float* loss_dev,
                    hipStream_t s, const float* weights, float* td_abs, bool fuse_update) {
  model_backward_dense(m, B, actions, y, loss_dev, s, weights, td_abs);
  model_backward_conv(m, table, B, s, fuse_update);
}

// the head and dense part of the backward: Huber (+ dz4), dW4 / db4 / loss, dW3 / db3 and dz3
void model_backward_dense(qlx_model* m, int B, const uint8_t* actions, const float* y, float* loss_dev, hipStream_t s,
                          const float* weights, float* td_abs) {
  m->f32 ? f32_backward_dense(m, B, actions, y, loss_dev, s, weights, td_abs)
         : bf16_backward_dense(m, B, actions, y, loss_dev, s, weights, td_abs);
}

void model_backward_dq(qlx_model* m, const uint8_t* const* table, int B, const float* dq, hipStream_t s, bool fuse_update) {
  model_backward_dq_dense(m, B, dq, s);
  model_backward_conv(m, table, B, s, fuse_update);
}

void model_backward_dq_dense(qlx_model* m, int B, const float* dq, hipStream_t s) {
  m->f32 ? f32_backward_dense_dq(m, B, dq, s) : bf16_backward_dense_dq(m, B, dq, s);
}

// the conv part of the backward (after model_backward_dense on the same batch): dz3 -> dz2 -> dz1 and the
// three conv weight gradients into m->d_grads
void model_backward_conv(qlx_model* m, const uint8_t* const* table, int B, hipStream_t s, bool fuse_update, hipEvent_t dense_ready,
                         float dense_scale) {
  m->f32 ? f32_backward_conv(m, table, B, s, fuse_update, dense_ready, dense_scale) : bf16_backward_conv(m, table, B, s);
  m->grads_filled = true;
  m->head_grads = false;   // (qlx_head_backward_dev sets it again after this call)
}

void model_gradient_replaced(qlx_model* m) { m->f32 ? f32_gradient_replaced(m) : bf16_gradient_replaced(m); }

void model_norms_dense(qlx_model* m, hipStream_t s, float scale) {
  if (m->f32) f32_norms(m, s, scale);   // reads the dense gradient only
}

void model_norms(qlx_model* m, hipStream_t s, float scale) { m->f32 ? f32_norms(m, s, scale) : bf16_norms(m, s, scale); }

void model_adam(qlx_model* m, hipStream_t s, float scale) {
  m->f32 ? f32_adam(m, s, scale) : bf16_adam(m, s, scale);
  m->fwd_reusable = false;   // the activations belong to the weights before this update
}

static void model_frame_table_from_host(qlx_model* m, const uint8_t* obs_host, int B) {
  model_workspace(m, B);
  const size_t bytes = (size_t)B * kFramePix * 4;
  DeviceBuffer<uint8_t> d_obs(bytes);
  QLX_HIP(hipMemcpyAsync(d_obs, obs_host, bytes, hipMemcpyHostToDevice, m->stream));
  hipLaunchKernelGGL(k_pack_obs, dim3((B * kFramePix + 255) / 256), dim3(256), 0, m->stream, d_obs, B, m->w.frames);
  hipLaunchKernelGGL(k_frame_table, dim3((B * 4 + 255) / 256), dim3(256), 0, m->stream, m->w.frames, B, m->w.table);
  QLX_HIP(hipGetLastError());
  QLX_HIP(hipStreamSynchronize(m->stream));
}

static void glorot_host(std::vector<float>& params, uint64_t seed) {
  const int fan_in[5] = {8 * 8 * 4, 4 * 4 * 32, 3 * 3 * 64, 3136, 512};
  const int fan_out[5] = {8 * 8 * 32, 4 * 4 * 64, 3 * 3 * 64, 512, 3};
  params.assign(kNumParams, 0.0f);
  int64_t off = 0;
  for (int v = 0; v < kNumVars; ++v) {
    if (v % 2 == 0) {
      const int l = v / 2;
      const float limit = std::sqrt(6.0f / (float)(fan_in[l] + fan_out[l]));
      RngStream s(seed, (uint32_t)v, 0, P_INIT);
      for (int i = 0; i < kVarSize[v]; ++i) params[off + i] = uniform_f32(s, -limit, limit);
    }
    off += kVarSize[v];
  }
}

}  // namespace qlx

using namespace qlx;

extern "C" {

int32_t qlx_model_num_vars(void) { return kNumVars; }

int32_t qlx_model_hparams(float* out) {
  return guard([&] {
    QLX_CHECK(out, QLX_E_INVALID, "null out");
    const qlx_model m;   // the defaults every created model starts from (no device state is touched)
    out[0] = m.lr; out[1] = m.beta1; out[2] = m.beta2; out[3] = m.eps; out[4] = m.clipnorm;
  });
}
int64_t qlx_model_var_size(int32_t v) { return (v >= 0 && v < kNumVars) ? kVarSize[v] : -1; }

int32_t qlx_model_create(int32_t arch, uint64_t seed, int32_t device, qlx_model** out) {
  return guard([&] {
    QLX_CHECK((arch == QLX_ARCH_NATURE_DQN || arch == QLX_ARCH_NATURE_DQN_BF16) && out, QLX_E_INVALID, "unknown model arch");
    current_device_checked(device);
    auto* m = new qlx_model;
    m->f32 = arch == QLX_ARCH_NATURE_DQN;
    try {   // a failure part-way releases what was built
      m->device = device;
      QLX_HIP(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
      const size_t pb = kNumParams * sizeof(float);
      m->d_params.alloc(kNumParams);
      m->d_m.alloc(kNumParams);
      m->d_v.alloc(kNumParams);
      m->d_grads.alloc(kNumParams);
      m->d_norms.alloc(16);
      m->f32 ? f32_create(m) : bf16_create(m);
      std::vector<float> params;
      glorot_host(params, seed);
      QLX_HIP(hipMemcpy(m->d_params, params.data(), pb, hipMemcpyHostToDevice));
      QLX_HIP(hipMemset(m->d_m, 0, pb));
      QLX_HIP(hipMemset(m->d_v, 0, pb));
      QLX_HIP(hipMemset(m->d_grads, 0, pb));
      model_pack(m);
      QLX_HIP(hipStreamSynchronize(m->stream));
    } catch (...) {
      qlx_model_destroy(m);
      throw;
    }
    *out = m;
  });
}

int32_t qlx_model_destroy(qlx_model* m) {
  return guard([&] {
    if (!m) return;
    QLX_CHECK(!m->head, QLX_E_STATE, "the model has a live head: qlx_head_destroy first");
    (void)hipSetDevice(m->device);
    (void)hipStreamSynchronize(m->stream);
    m->f32 ? f32_destroy(m) : bf16_destroy(m);
    if (m->own_stream) (void)hipStreamDestroy(m->stream);
    if (m->dev_event) (void)hipEventDestroy(m->dev_event);
    delete m;
  });
}

int32_t qlx_model_get_var(qlx_model* m, int32_t var, int32_t which, float* out) {
  return guard([&] {
    QLX_CHECK(m && out && var >= 0 && var < kNumVars && which >= 0 && which <= 2, QLX_E_INVALID, "bad argument");
    QLX_HIP(hipSetDevice(m->device));
    QLX_HIP(hipStreamSynchronize(m->stream));
    const float* src = (which == 0 ? m->d_params : which == 1 ? m->d_m : m->d_v) + var_offset(var);
    QLX_HIP(hipMemcpy(out, src, kVarSize[var] * sizeof(float), hipMemcpyDeviceToHost));
  });
}

int32_t qlx_model_set_var(qlx_model* m, int32_t var, int32_t which, const float* in) {
  return guard([&] {
    QLX_CHECK(m && in && var >= 0 && var < kNumVars && which >= 0 && which <= 2, QLX_E_INVALID, "bad argument");
    QLX_HIP(hipSetDevice(m->device));
    QLX_HIP(hipStreamSynchronize(m->stream));
    float* dst = (which == 0 ? m->d_params : which == 1 ? m->d_m : m->d_v) + var_offset(var);
    QLX_HIP(hipMemcpy(dst, in, kVarSize[var] * sizeof(float), hipMemcpyHostToDevice));
    if (which == 0) {
      model_pack(m);
      QLX_HIP(hipStreamSynchronize(m->stream));
    }
  });
}

int64_t qlx_model_iterations(qlx_model* m) { return m ? m->iterations : -1; }

int32_t qlx_model_copy_weights(qlx_model* dst, const qlx_model* src) {
  return guard([&] {
    QLX_CHECK(dst && src, QLX_E_INVALID, "null model");
    QLX_HIP(hipSetDevice(dst->device));
    QLX_HIP(hipStreamSynchronize(src->stream));
    QLX_HIP(hipMemcpyAsync(dst->d_params, src->d_params, kNumParams * sizeof(float), hipMemcpyDeviceToDevice, dst->stream));
    model_pack(dst);
    QLX_HIP(hipStreamSynchronize(dst->stream));
  });
}

int32_t qlx_model_predict(qlx_model* m, const uint8_t* obs, uint32_t n, float* q_out, uint8_t* actions) {
  return guard([&] {
    QLX_CHECK(m && obs && n > 0, QLX_E_INVALID, "bad argument");
    QLX_HIP(hipSetDevice(m->device));
    model_frame_table_from_host(m, obs, (int)n);
    model_forward_trunk(m, m->w.table, (int)n, m->stream);
    Fc2Args a = fc2_args(m, (int)n);
    a.argmax = m->w.argmax;
    model_head(m, 1, a, (int)n, m->stream);
    if (q_out) QLX_HIP(hipMemcpyAsync(q_out, m->w.q, n * 3 * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    if (actions) QLX_HIP(hipMemcpyAsync(actions, m->w.argmax, n, hipMemcpyDeviceToHost, m->stream));
    QLX_HIP(hipStreamSynchronize(m->stream));
  });
}

int32_t qlx_model_batch_max_q(qlx_model* m, const uint8_t* obs, uint32_t n, float* out) {
  return guard([&] {
    QLX_CHECK(m && obs && out && n > 0, QLX_E_INVALID, "bad argument");
    QLX_HIP(hipSetDevice(m->device));
    model_frame_table_from_host(m, obs, (int)n);
    model_forward_trunk(m, m->w.table, (int)n, m->stream);
    // y = 0 + max * 1 with done = 0: the bare reduce_max of the reference signature
    QLX_HIP(hipMemsetAsync(m->w.rew, 0, n * 4, m->stream));
    QLX_HIP(hipMemsetAsync(m->w.done, 0, n, m->stream));
    Fc2Args a = fc2_args(m, (int)n);
    a.rewards = m->w.rew; a.dones = m->w.done; a.gamma = 1.0f; a.y_out = m->w.y;
    model_head(m, 2, a, (int)n, m->stream);
    QLX_HIP(hipMemcpyAsync(out, m->w.y, n * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    QLX_HIP(hipStreamSynchronize(m->stream));
  });
}

int32_t qlx_model_train(qlx_model* m, const uint8_t* obs, const uint8_t* actions, const float* y, uint32_t B,
                        float* loss_out, float* grads_out, float* norms_out) {
  return guard([&] {
    QLX_CHECK(m && obs && actions && y && B > 0, QLX_E_INVALID, "bad argument");
    for (uint32_t b = 0; b < B; ++b) QLX_CHECK(actions[b] < kActions, QLX_E_INVALID, "action out of range");
    QLX_HIP(hipSetDevice(m->device));
    model_frame_table_from_host(m, obs, (int)B);
    hipStream_t s = m->stream;
    QLX_HIP(hipMemcpyAsync(m->w.act, actions, B, hipMemcpyHostToDevice, s));
    QLX_HIP(hipMemcpyAsync(m->w.y, y, B * 4, hipMemcpyHostToDevice, s));
    model_forward_trunk(m, m->w.table, (int)B, s);
    model_backward(m, m->w.table, (int)B, m->w.act, m->w.y, m->w.loss, s, nullptr, nullptr, true);
    if (grads_out) QLX_HIP(hipMemcpyAsync(grads_out, m->d_grads, kNumParams * 4, hipMemcpyDeviceToHost, s));
    model_norms(m, s, 1.0f);
    model_adam(m, s, 1.0f);
    if (norms_out) QLX_HIP(hipMemcpyAsync(norms_out, m->d_norms, kNumVars * 4, hipMemcpyDeviceToHost, s));
    if (loss_out) QLX_HIP(hipMemcpyAsync(loss_out, m->w.loss, 4, hipMemcpyDeviceToHost, s));
    QLX_HIP(hipStreamSynchronize(s));
  });
}

// The update tail alone on a given gradient (test hook of the data-parallel tail, whose all-reduced gradient is scaled by
// 1 / world): clip_by_norm of (grads x scale) per variable + legacy Adam, exactly as learner_update runs them after an
// all-reduce (model_norms, then model_adam at that scale).  fp32: the same two launches as a rank's DP tail; bf16: the
// explicit sum-of-squares pass (the backward's fused partials do not belong to this gradient) and the Adam launch.
int32_t qlx_model_apply_gradient(qlx_model* m, const float* grads, float scale, float* norms_out) {
  return guard([&] {
    QLX_CHECK(m && grads, QLX_E_INVALID, "null argument");
    QLX_CHECK(std::isfinite(scale) && scale > 0.0f, QLX_E_INVALID, "scale must be finite and > 0");
    QLX_HIP(hipSetDevice(m->device));
    hipStream_t s = m->stream;
    model_workspace(m, std::max(m->ws_batch, 1));   // (the norm partial buffers)
    QLX_HIP(hipMemcpyAsync(m->d_grads, grads, kNumParams * 4, hipMemcpyHostToDevice, s));
    m->grads_filled = true;
    m->head_grads = false;
    model_gradient_replaced(m);
    model_norms(m, s, scale);
    model_adam(m, s, scale);
    if (norms_out) QLX_HIP(hipMemcpyAsync(norms_out, m->d_norms, kNumVars * 4, hipMemcpyDeviceToHost, s));
    QLX_HIP(hipStreamSynchronize(s));
  });
}

int32_t qlx_model_last_activation(qlx_model* m, int32_t layer, float* out) {
  return guard([&] {
    QLX_CHECK(m && out && layer >= 1 && layer <= 4 && m->ws_batch > 0, QLX_E_INVALID, "bad argument");
    QLX_HIP(hipSetDevice(m->device));
    m->f32 ? f32_last_activation(m, layer, out) : bf16_last_activation(m, layer, out);
  });
}

int32_t qlx_model_write_checkpoint(qlx_model* m, const char* path) {
  return guard([&] {
    QLX_CHECK(m && path, QLX_E_INVALID, "bad argument");
    QLX_HIP(hipStreamSynchronize(m->stream));
    std::vector<float> buf(kNumParams * 3);
    QLX_HIP(hipMemcpy(buf.data(), m->d_params, kNumParams * 4, hipMemcpyDeviceToHost));
    QLX_HIP(hipMemcpy(buf.data() + kNumParams, m->d_m, kNumParams * 4, hipMemcpyDeviceToHost));
    QLX_HIP(hipMemcpy(buf.data() + 2 * kNumParams, m->d_v, kNumParams * 4, hipMemcpyDeviceToHost));
    FILE* f = std::fopen(path, "wb");
    QLX_CHECK(f, QLX_E_IO, std::string("cannot open ") + path);
    const char magic[8] = {'Q', 'L', 'X', 'C', 'K', 'P', 'T', '1'};
    const int64_t hdr[2] = {kNumParams, m->iterations};
    bool ok = std::fwrite(magic, 1, 8, f) == 8 && std::fwrite(hdr, 8, 2, f) == 2 &&
              std::fwrite(buf.data(), 4, buf.size(), f) == buf.size();
    ok = (std::fclose(f) == 0) && ok;
    QLX_CHECK(ok, QLX_E_IO, "checkpoint write failed");
  });
}

// weights, Adam slots and the iteration count as read from a file, onto the device
static void model_restore(qlx_model* m, const float* w, const float* mm, const float* vv, int64_t iterations);

}  // extern "C"

namespace qlx {
void model_state_get(qlx_model* m, float* out3, int64_t* iterations) {
  QLX_HIP(hipSetDevice(m->device));
  QLX_HIP(hipStreamSynchronize(m->stream));
  QLX_HIP(hipMemcpy(out3, m->d_params, kNumParams * 4, hipMemcpyDeviceToHost));
  QLX_HIP(hipMemcpy(out3 + kNumParams, m->d_m, kNumParams * 4, hipMemcpyDeviceToHost));
  QLX_HIP(hipMemcpy(out3 + 2 * kNumParams, m->d_v, kNumParams * 4, hipMemcpyDeviceToHost));
  *iterations = m->iterations;
}
void model_state_put(qlx_model* m, const float* in3, int64_t iterations) {
  model_restore(m, in3, in3 + kNumParams, in3 + 2 * kNumParams, iterations);
}
}  // namespace qlx

extern "C" {

static void model_restore(qlx_model* m, const float* w, const float* mm, const float* vv, int64_t iterations) {
  QLX_HIP(hipSetDevice(m->device));
  QLX_HIP(hipStreamSynchronize(m->stream));
  QLX_HIP(hipMemcpy(m->d_params, w, kNumParams * 4, hipMemcpyHostToDevice));
  QLX_HIP(hipMemcpy(m->d_m, mm, kNumParams * 4, hipMemcpyHostToDevice));
  QLX_HIP(hipMemcpy(m->d_v, vv, kNumParams * 4, hipMemcpyHostToDevice));
  m->iterations = iterations;
  model_pack(m);
  QLX_HIP(hipStreamSynchronize(m->stream));
}

int32_t qlx_model_load_tf(qlx_model* m, const char* prefix) {
  return guard([&] {
    QLX_CHECK(m && prefix, QLX_E_INVALID, "null argument");
    std::vector<float> w, mm, vv;
    int64_t it = 0;
    load_keras_bundle(prefix, 5, kVarSize, w, mm, vv, &it);
    model_restore(m, w.data(), mm.data(), vv.data(), it);
  });
}

int32_t qlx_model_read_checkpoint(qlx_model* m, const char* path) {
  return guard([&] {
    QLX_CHECK(m && path, QLX_E_INVALID, "bad argument");
    FILE* f = std::fopen(path, "rb");
    QLX_CHECK(f, QLX_E_IO, std::string("cannot open ") + path);
    char magic[8];
    int64_t hdr[2];
    std::vector<float> buf(kNumParams * 3);
    bool ok = std::fread(magic, 1, 8, f) == 8 && std::memcmp(magic, "QLXCKPT1", 8) == 0 && std::fread(hdr, 8, 2, f) == 2 &&
              hdr[0] == kNumParams && std::fread(buf.data(), 4, buf.size(), f) == buf.size();
    std::fclose(f);
    QLX_CHECK(ok, QLX_E_IO, "not a qlx checkpoint");
    model_restore(m, buf.data(), buf.data() + kNumParams, buf.data() + 2 * kNumParams, hdr[1]);
  });
}

int32_t qlx_model_sync(qlx_model* m) {
  return guard([&] {
    QLX_CHECK(m, QLX_E_INVALID, "null model");
    QLX_HIP(hipStreamSynchronize(m->stream));
    if (!m->d_dev_flag) return;   // only the _dev calls (model_dev.hip) set the flag, and they need a reserve
    QLX_HIP(hipSetDevice(m->device));
    uint32_t flag = 0;
    QLX_HIP(hipMemcpy(&flag, m->d_dev_flag, 4, hipMemcpyDeviceToHost));
    if (flag) QLX_HIP(hipMemset(m->d_dev_flag, 0, 4));
    QLX_CHECK(flag == 0, QLX_E_INVALID,
              flag == 1 ? "replay index out of range (>= len) in a device call"
                        : flag == 2 ? "action out of range (>= 3) in a device call"
                                    : "replay index out of range (>= len) and action out of range (>= 3) in device calls");
  });
}

}  // extern "C"
