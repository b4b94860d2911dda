// Device-tensor entry points of the Q-network (gfx950): the forward and the whole update on states that are already in
// device memory, enqueue only.  The model layer takes a table of four frame pointers per sample; this file
// builds that table from each of the three state sources and hands it to model_forward_trunk / model_head / model_backward.
//
// Dense states: k_pack_states, the mirror image of batch_dev.hip's k_unpack_states.  A ring frame is 441 chunks of 16 B, chunk
// (X, Y) a 4 x 4 pixel block whose dword r is the four y-consecutive pixels of row x = 4X + r, that is dword
// (4X + r) * 21 + Y of the dense [x][y] image counted in dwords.  One 256-thread workgroup per sample loads the state with
// coalesced 16-byte loads (all seven of a lane in flight), lays the four dense images out in LDS
//   NCHW_TIME: an input chunk is four consecutive dwords of one image: ds_write_b128 as it is;
//   NHWC_SLOT: input chunk q is the four pixels of image dword q in all four slots: a 4 x 4 byte transpose (v_perm_b32) in
//   registers, then dword q of each image (four ds_write_b32, consecutive over the lanes);
// and reads each output chunk back as four dwords at stride 21 for one coalesced 16-byte store.
// LDS banks: the stride-21 ds_read_b32 of a wave go to consecutive dwords except where Y wraps (address + 63: two lanes of 32
// on one bank, once or twice per half wave); the writes are consecutive per lane.
// Replay indices and an env's ring move no state bytes: k_state_table_* write frame pointers only.
#include <hip/hip_runtime.h>

#include "objects.h"
#include "qnet.h"
#include "replay_dev.h"

namespace qlx {

ReplayView replay_view(const qlx_replay* rb);   // replay.hip

constexpr int kChunks = kFramePix / 16;             // 441 16-byte chunks per frame
constexpr int kStateBytes = kSlots * kFramePix;     // 28,224
constexpr int kStateChunks = kSlots * kChunks;      // 1,764
constexpr int kPackIters = (kStateChunks + 255) / 256;   // 7 chunks per lane
constexpr uint32_t kMaxStates = 8192;   // one fp32 forward chunk (kF32FwdChunk)
constexpr uint32_t kMaxTrain = 4096;
constexpr uint32_t kFlagIndex = 1u, kFlagAction = 2u;
static_assert(kMaxStates == (uint32_t)kF32FwdChunk, "a _dev forward is one chunk");

// D byte i = byte sel[i] of the eight bytes {lo: 0-3, hi: 4-7}
__device__ __forceinline__ uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel) { return __builtin_amdgcn_perm(hi, lo, sel); }

template <int LAYOUT>
__global__ __launch_bounds__(256) void k_pack_states(const uint8_t* __restrict__ obs, uint8_t* __restrict__ frames,
                                                     const uint8_t** __restrict__ table) {
  __shared__ __attribute__((aligned(16))) uint32_t img[kStateChunks * 4];   // four dense [x][y] images, 28,224 B
  const int tid = threadIdx.x;
  const size_t b = blockIdx.x;
  const uint4* in = reinterpret_cast<const uint4*>(obs + b * kStateBytes);
  uint4 v[kPackIters];
#pragma unroll
  for (int k = 0; k < kPackIters; ++k) {
    const int i = tid + 256 * k;
    v[k] = i < kStateChunks ? in[i] : make_uint4(0, 0, 0, 0);
  }
#pragma unroll
  for (int k = 0; k < kPackIters; ++k) {
    const int i = tid + 256 * k;
    if (i < kStateChunks) {
      if (LAYOUT == QLX_OBS_NCHW_TIME) {
        reinterpret_cast<uint4*>(img)[i] = v[k];
      } else {
        // v.{x,y,z,w} = pixel y0 + {0..3}, byte s = slot s; image s gets (x.s, y.s, z.s, w.s)
        const uint32_t lo01 = perm(v[k].y, v[k].x, 0x05010400u), hi01 = perm(v[k].y, v[k].x, 0x07030602u);
        const uint32_t lo23 = perm(v[k].w, v[k].z, 0x05010400u), hi23 = perm(v[k].w, v[k].z, 0x07030602u);
        img[i] = perm(lo23, lo01, 0x05040100u);
        img[kStateChunks + i] = perm(lo23, lo01, 0x07060302u);
        img[2 * kStateChunks + i] = perm(hi23, hi01, 0x05040100u);
        img[3 * kStateChunks + i] = perm(hi23, hi01, 0x07060302u);
      }
    }
  }
  __syncthreads();
  uint4* out = reinterpret_cast<uint4*>(frames + b * kStateBytes);
#pragma unroll
  for (int k = 0; k < kPackIters; ++k) {
    const int i = tid + 256 * k;
    if (i < kStateChunks) {
      const int c = i / kChunks, ch = i - c * kChunks;
      const int X = ch / kBlocks, Y = ch - X * kBlocks;
      const uint32_t* s = img + c * kStateChunks + 4 * X * kBlocks + Y;
      out[i] = make_uint4(s[0], s[kBlocks], s[2 * kBlocks], s[3 * kBlocks]);
    }
  }
  if (tid < kSlots) table[b * kSlots + tid] = frames + (b * kSlots + tid) * kFramePix;
}

// frame pointers of the transitions at idx (which: 0 = s, 1 = s'), in the layout's channel order; an index >= len reads
// nothing: four null pointers (conv1 reads a null frame as zeros) and the flag
__global__ __launch_bounds__(256) void k_state_table_replay(ReplayView r, const uint64_t* idx, uint32_t n, int which, int time,
                                                            const uint8_t** table, uint32_t* flag) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  const uint64_t i = idx[b];
  const uint8_t* f[4] = {nullptr, nullptr, nullptr, nullptr};
  if (i >= r.len) {
    atomicOr(flag, kFlagIndex);
  } else {
    const uint8_t* slot[4];
    replay_frames(r, i, which, slot);
    // ring slot of episode step m is (m - 1) & 3: s' (step k newest) starts at slot k & 3, s (step k - 1 newest) at (k - 1) & 3
    const uint32_t first = time ? r.epstep[(r.total - r.len + i) % r.cap] + (uint32_t)which - 1u : 0u;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const uint32_t j = (first + c) & 3u;
      f[c] = j == 0 ? slot[0] : j == 1 ? slot[1] : j == 2 ? slot[2] : slot[3];
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) table[(size_t)b * 4 + c] = f[c];
}

// frame pointers into an env's ring: channel c is ring slot c, or (next_slot + c) & 3 oldest first
__global__ __launch_bounds__(256) void k_state_table_env(const uint8_t* obs, const qlx_breakout_state* st, uint32_t n, int time,
                                                         const uint8_t** table) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const uint32_t first = time ? st[e].next_slot : 0u;
#pragma unroll
  for (int c = 0; c < 4; ++c) table[(size_t)e * 4 + c] = obs + ((size_t)e * kSlots + ((first + c) & 3u)) * kFramePix;
}

// the caller's actions into the model's scratch, 0 (and the flag) in place of a value the training head cannot index
__global__ __launch_bounds__(256) void k_train_args(const uint8_t* actions, uint32_t B, uint8_t* act, uint32_t* flag) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  uint8_t a = actions[b];
  if (a >= kActions) {
    a = 0;
    atomicOr(flag, kFlagAction);
  }
  act[b] = a;
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// everything about a state source that can be judged without reading a handle
void check_source(const qlx_states_dev* s) {
  QLX_CHECK(s, QLX_E_INVALID, "null src");
  QLX_CHECK(!(s->indices && !s->replay), QLX_E_INVALID, "src->indices without src->replay");
  QLX_CHECK(!(s->replay && !s->indices), QLX_E_INVALID, "src->replay without src->indices");
  const int sources = (s->obs ? 1 : 0) + (s->replay ? 1 : 0) + (s->env ? 1 : 0);
  QLX_CHECK(sources != 0, QLX_E_INVALID, "no state source: set src->obs, src->replay + indices or src->env");
  QLX_CHECK(sources == 1, QLX_E_INVALID, "more than one state source in src");
  QLX_CHECK(s->layout == QLX_OBS_NHWC_SLOT || s->layout == QLX_OBS_NCHW_TIME, QLX_E_INVALID, "unknown src->layout");
  QLX_CHECK(s->which == 0 || s->which == 1, QLX_E_INVALID, "src->which must be 0 or 1");
  QLX_CHECK(aligned16(s->obs), QLX_E_INVALID, "src->obs is not 16-byte aligned");
}

// the checks that read the handles: nothing is launched before all of them passed
void check_handles(const qlx_model* m, const qlx_states_dev& s, uint32_t n) {
  QLX_CHECK(n <= m->dev_reserved, QLX_E_STATE, "n is above the reserved size: qlx_model_reserve first");
  QLX_CHECK(!s.replay || s.replay->device == m->device, QLX_E_INVALID, "src->replay and the model are on different devices");
  QLX_CHECK(!s.env || s.env->device == m->device, QLX_E_INVALID, "src->env and the model are on different devices");
  QLX_CHECK(!s.env || s.env->n == n, QLX_E_INVALID, "n is not src->env's env count");
}

// m->w.table for the n states of `s`, enqueued on the model's stream
const uint8_t* const* states_table(qlx_model* m, const qlx_states_dev& s, uint32_t n) {
  hipStream_t st = m->stream;
  const int time = s.layout == QLX_OBS_NCHW_TIME;
  if (s.obs) {
    if (time)
      hipLaunchKernelGGL(k_pack_states<QLX_OBS_NCHW_TIME>, dim3(n), dim3(256), 0, st, s.obs, m->w.frames, m->w.table);
    else
      hipLaunchKernelGGL(k_pack_states<QLX_OBS_NHWC_SLOT>, dim3(n), dim3(256), 0, st, s.obs, m->w.frames, m->w.table);
  } else if (s.replay) {
    hipLaunchKernelGGL(k_state_table_replay, dim3((n + 255) / 256), dim3(256), 0, st, replay_view(s.replay), s.indices, n, s.which,
                       time, m->w.table, m->d_dev_flag.get());
  } else {
    hipLaunchKernelGGL(k_state_table_env, dim3((n + 255) / 256), dim3(256), 0, st, s.env->d_obs.get(), s.env->d_state.get(), n, time,
                       m->w.table);
  }
  QLX_HIP(hipGetLastError());
  return m->w.table;
}

}  // namespace qlx

using namespace qlx;

extern "C" {

int32_t qlx_model_stream(qlx_model* m, void** out) {
  return guard([&] {
    QLX_CHECK(m, QLX_E_INVALID, "null model");
    QLX_CHECK(out, QLX_E_INVALID, "null hip_stream_out");
    *out = m->stream;
  });
}

// (neither backend keeps a stream of its own: every launch takes the stream it is given or reads m->stream at the call)
int32_t qlx_model_share_stream(qlx_model* m, qlx_env* e) {
  return guard([&] {
    QLX_CHECK(m, QLX_E_INVALID, "null model");
    QLX_CHECK(e, QLX_E_INVALID, "null env");
    QLX_CHECK(m->device == e->device, QLX_E_INVALID, "model and env are on different devices");
    if (m->stream == e->stream) return;
    QLX_HIP(hipSetDevice(m->device));
    QLX_HIP(hipStreamSynchronize(m->stream));
    adopt_stream(m, e->stream);
  });
}

int32_t qlx_model_reserve(qlx_model* m, uint32_t max_n) {
  return guard([&] {
    QLX_CHECK(m, QLX_E_INVALID, "null model");
    QLX_CHECK(max_n > 0 && max_n <= kMaxStates, QLX_E_INVALID, "max_n must be in 1..8192");
    QLX_HIP(hipSetDevice(m->device));
    model_workspace(m, (int)max_n);   // (grows only; synchronises when it does)
    if (!m->d_dev_flag) {
      QLX_HIP(hipStreamSynchronize(m->stream));
      m->d_dev_flag.alloc(4);
      m->d_dev_act.alloc(kMaxTrain);
      m->d_dev_zero.alloc(kMaxStates);
      QLX_HIP(hipMemset(m->d_dev_flag, 0, m->d_dev_flag.bytes()));
      QLX_HIP(hipMemset(m->d_dev_zero, 0, m->d_dev_zero.bytes()));
    }
    QLX_HIP(hipStreamSynchronize(m->stream));
    if (max_n > m->dev_reserved) m->dev_reserved = max_n;
  });
}

int32_t qlx_model_q_dev(qlx_model* m, const qlx_states_dev* src, uint32_t n, float* d_q, uint8_t* d_actions, float* d_max_q) {
  return guard([&] {
    QLX_CHECK(m, QLX_E_INVALID, "null model");
    check_source(src);
    QLX_CHECK(n > 0 && n <= kMaxStates, QLX_E_INVALID, "n must be in 1..8192");
    QLX_CHECK(d_q || d_actions || d_max_q, QLX_E_INVALID, "d_q, d_actions and d_max_q are all null");
    const qlx_states_dev s = *src;
    check_handles(m, s, n);
    QLX_HIP(hipSetDevice(m->device));
    hipStream_t st = m->stream;
    const uint8_t* const* table = states_table(m, s, n);
    model_forward_trunk(m, table, (int)n, st);
    if (d_q || d_actions) {
      Fc2Args a = fc2_args(m, (int)n);
      a.q = d_q;
      a.argmax = d_actions ? d_actions : m->w.argmax;
      model_head(m, 1, a, (int)n, st);
    }
    if (d_max_q) {
      // y = 0 + max * 1 with done = 0 (qlx_model_batch_max_q); the zero words serve as rewards and as dones
      Fc2Args a = fc2_args(m, (int)n);
      a.q = nullptr;
      a.rewards = m->d_dev_zero;
      a.dones = reinterpret_cast<const uint8_t*>(m->d_dev_zero.get());
      a.gamma = 1.0f;
      a.y_out = d_max_q;
      model_head(m, 2, a, (int)n, st);
    }
  });
}

int32_t qlx_model_train_dev(qlx_model* m, const qlx_states_dev* src, const uint8_t* d_actions, const float* d_y,
                            const float* d_weights, uint32_t batch, float* d_loss, float* d_td_abs) {
  return guard([&] {
    QLX_CHECK(m, QLX_E_INVALID, "null model");
    check_source(src);
    QLX_CHECK(d_actions, QLX_E_INVALID, "null d_actions");
    QLX_CHECK(d_y, QLX_E_INVALID, "null d_y");
    QLX_CHECK(batch > 0 && batch <= kMaxTrain, QLX_E_INVALID, "batch must be in 1..4096");
    const qlx_states_dev s = *src;
    check_handles(m, s, batch);
    QLX_HIP(hipSetDevice(m->device));
    hipStream_t st = m->stream;
    const int B = (int)batch;
    hipLaunchKernelGGL(k_train_args, dim3((batch + 255) / 256), dim3(256), 0, st, d_actions, batch, m->d_dev_act.get(),
                       m->d_dev_flag.get());
    QLX_HIP(hipGetLastError());
    const uint8_t* const* table = states_table(m, s, batch);
    model_forward_trunk(m, table, B, st);
    model_backward(m, table, B, m->d_dev_act, d_y, d_loss ? d_loss : m->w.loss, st, d_weights, d_td_abs, true);
    model_norms(m, st, 1.0f);
    model_adam(m, st, 1.0f);
  });
}

int32_t qlx_model_forward_ticket(qlx_model* m, uint64_t* ticket_out) {
  return guard([&] {
    QLX_CHECK(m, QLX_E_INVALID, "null model");
    QLX_CHECK(ticket_out, QLX_E_INVALID, "null ticket_out");
    *ticket_out = m->fwd_ticket;
  });
}

// The last forward's activations serve when the ticket is that forward's, it ran over `batch` samples of the model's own
// table (a _dev or host call built it, and it is still in place), it stored its activations, and neither the weights nor
// the workspace changed since (model_forward_trunk / model_adam / model_pack / model_workspace keep fwd_reusable).  The
// bf16 forward may have left a4 as pending fc1 partials: either way the dq head finishes a4 exactly as the forward's head
// did (fc2_args), so both ways give the same gradient.
int32_t qlx_model_backward_dev(qlx_model* m, const qlx_states_dev* src, const float* d_dq, uint32_t batch, uint64_t ticket) {
  return guard([&] {
    QLX_CHECK(m, QLX_E_INVALID, "null model");
    check_source(src);
    QLX_CHECK(d_dq, QLX_E_INVALID, "null d_dq");
    QLX_CHECK(batch > 0 && batch <= kMaxTrain, QLX_E_INVALID, "batch must be in 1..4096");
    const qlx_states_dev s = *src;
    check_handles(m, s, batch);
    QLX_HIP(hipSetDevice(m->device));
    hipStream_t st = m->stream;
    const int B = (int)batch;
    const bool reuse = ticket != 0 && ticket == m->fwd_ticket && m->fwd_reusable && m->last_batch == B && m->fwd_table == m->w.table;
    if (!reuse) model_forward_trunk(m, states_table(m, s, batch), B, st);
    model_backward_dq(m, m->w.table, B, d_dq, st, false);
  });
}

int32_t qlx_model_step_dev(qlx_model* m, uint32_t flags) {
  return guard([&] {
    QLX_CHECK(m, QLX_E_INVALID, "null model");
    QLX_CHECK((flags & ~(uint32_t)QLX_STEP_GRADS_WRITTEN) == 0, QLX_E_INVALID, "unknown flags");
    QLX_CHECK(m->grads_filled, QLX_E_STATE, "no gradient yet: qlx_model_backward_dev (or a train call) first");
    QLX_HIP(hipSetDevice(m->device));
    hipStream_t st = m->stream;
    if (flags & QLX_STEP_GRADS_WRITTEN) model_gradient_replaced(m);
    model_norms(m, st, 1.0f);
    model_adam(m, st, 1.0f);
    if (m->head && m->head_grads) head_step(m->head, st);   // the gradient came from qlx_head_backward_dev
  });
}

int32_t qlx_model_grads_dev(qlx_model* m, float** d_grads_out, uint64_t* count_out) {
  return guard([&] {
    QLX_CHECK(m, QLX_E_INVALID, "null model");
    QLX_CHECK(d_grads_out, QLX_E_INVALID, "null d_grads_out");
    QLX_CHECK(count_out, QLX_E_INVALID, "null count_out");
    *d_grads_out = m->d_grads.get();
    *count_out = (uint64_t)kNumParams;
  });
}

int32_t qlx_model_copy_weights_dev(qlx_model* dst, qlx_model* src) {
  return guard([&] {
    QLX_CHECK(dst, QLX_E_INVALID, "null dst");
    QLX_CHECK(src, QLX_E_INVALID, "null src");
    QLX_CHECK(dst->device == src->device, QLX_E_INVALID, "dst and src are on different devices");
    if (dst == src) return;
    QLX_HIP(hipSetDevice(dst->device));
    const bool two = dst->stream != src->stream;
    if (two) {
      if (!dst->dev_event) QLX_HIP(hipEventCreateWithFlags(&dst->dev_event, hipEventDisableTiming));
      QLX_HIP(hipEventRecord(dst->dev_event, src->stream));
      QLX_HIP(hipStreamWaitEvent(dst->stream, dst->dev_event, 0));
    }
    QLX_HIP(hipMemcpyAsync(dst->d_params, src->d_params, kNumParams * sizeof(float), hipMemcpyDeviceToDevice, dst->stream));
    model_pack(dst);
    if (two) {   // src's later updates write its weights: behind the copy
      QLX_HIP(hipEventRecord(dst->dev_event, dst->stream));
      QLX_HIP(hipStreamWaitEvent(src->stream, dst->dev_event, 0));
    }
  });
}

}  // extern "C"
