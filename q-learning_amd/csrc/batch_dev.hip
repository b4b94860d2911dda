// Device-tensor entry points of the env and the replay (gfx950): dense states and n-step batches written straight into
// caller-owned device memory, enqueue only.
//
// One unpack kernel serves both sources.  A state is four frames in the ring's space-to-depth layout (441 chunks of 16 B,
// each a 4 x 4 pixel block: qlx_internal.h s2d_offset); one 256-thread workgroup per (sample, state) loads them with
// coalesced 16-byte loads and writes each chunk's four dwords (dword r = the four y-consecutive pixels of row x = 4X + r)
// to LDS at dword (4X + r) * 21 + Y, which is the dense [x][y] image counted in dwords.  From that image
//   NCHW_TIME is a straight copy: output chunk i of the state is LDS chunk i (ds_read_b128, 16-byte stores);
//   NHWC_SLOT chunk d (four pixels x four slots) is dword d of each of the four images and a 4 x 4 byte transpose
//   (v_perm_b32) in registers.
// LDS banks: the ds_write_b32 of a wave go to consecutive dwords except where Y wraps (two lanes of 32 on one bank, which
// a ds_write_b32 absorbs); both reads are consecutive per lane.  The frame pointers are uniform over the workgroup; a frame
// the episode does not have yet is zero-filled without a load.
#include <hip/hip_runtime.h>

#include <cmath>

#include "objects.h"
#include "replay_dev.h"

namespace qlx {

ReplayView replay_view(const qlx_replay* rb);   // replay.hip

constexpr int kChunks = kFramePix / 16;             // 441 16-byte chunks per frame
constexpr int kStateBytes = kSlots * kFramePix;     // 28,224
constexpr int kStateChunks = kSlots * kChunks;      // 1,764
constexpr uint32_t kMaxBatch = 4096;
constexpr uint64_t kBadIndex = ~0ull;

struct EnvSource {
  const uint8_t* obs;               // [n][4][7056] ring frames
  const qlx_breakout_state* st;
  uint8_t* out;
};

struct ReplaySource {
  ReplayView r;
  const uint64_t* idx;    // [B] logical indices: the transitions whose s is asked for
  const uint64_t* last;   // [B] last index of each window (k_batch_meta): the transitions whose s' is asked for
  uint8_t* out[2];        // s, s'
  int which0;             // blockIdx.y = 0 is this state (0 = s, 1 = s')
  uint32_t* flag;
};

// the four frames of this workgroup's state in output order (TIME: oldest first, else by ring slot), null = zero frame
template <bool TIME>
__device__ __forceinline__ uint8_t* state_frames(const EnvSource& src, const uint8_t* f[4]) {
  const uint32_t e = blockIdx.x;
  const uint32_t first = TIME ? src.st[e].next_slot : 0u;
#pragma unroll
  for (int c = 0; c < 4; ++c) f[c] = src.obs + ((size_t)e * kSlots + ((first + c) & 3u)) * kFramePix;
  return src.out + (size_t)e * kStateBytes;
}

template <bool TIME>
__device__ __forceinline__ uint8_t* state_frames(const ReplaySource& src, const uint8_t* f[4]) {
  const uint32_t b = blockIdx.x;
  const int which = src.which0 + (int)blockIdx.y;
  const uint64_t i = which ? src.last[b] : src.idx[b];
  uint8_t* out = src.out[which] + (size_t)b * kStateBytes;
  if (i >= src.r.len) {   // nothing is read for it: a zero state and the sticky flag
    if (threadIdx.x == 0) atomicOr(src.flag, 1u);
#pragma unroll
    for (int c = 0; c < 4; ++c) f[c] = nullptr;
    return out;
  }
  const uint8_t* slot[4];
  replay_frames(src.r, i, which, slot);
  if (TIME) {
    // ring slot of episode step m is (m - 1) & 3: s' (step k newest) starts at slot k & 3, s (step k - 1 newest) at (k - 1) & 3
    const uint32_t k = src.r.epstep[(src.r.total - src.r.len + i) % src.r.cap];
    const uint32_t first = k + (uint32_t)which - 1u;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const uint32_t j = (first + c) & 3u;
      f[c] = j == 0 ? slot[0] : j == 1 ? slot[1] : j == 2 ? slot[2] : slot[3];
    }
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) f[c] = slot[c];
  }
  return out;
}

// D byte i = byte sel[i] of the eight bytes {lo: 0-3, hi: 4-7}
__device__ __forceinline__ uint32_t byte_perm(uint32_t hi, uint32_t lo, uint32_t sel) { return __builtin_amdgcn_perm(hi, lo, sel); }

template <int LAYOUT, class Source>
__global__ __launch_bounds__(256) void k_unpack_states(Source src) {
  __shared__ __attribute__((aligned(16))) uint32_t img[kStateChunks * 4];   // four dense [x][y] images, 28,224 B
  const int tid = threadIdx.x;
  const uint8_t* f[4];
  uint8_t* out = state_frames<LAYOUT == QLX_OBS_NCHW_TIME>(src, f);
  const bool second = tid + 256 < kChunks;
  uint4 v[4][2];
#pragma unroll
  for (int c = 0; c < 4; ++c) {   // all eight loads of a lane in flight before the first LDS write
    v[c][0] = v[c][1] = make_uint4(0, 0, 0, 0);
    if (f[c]) {
      const uint4* p = reinterpret_cast<const uint4*>(f[c]);
      v[c][0] = p[tid];
      if (second) v[c][1] = p[tid + 256];
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int ch = tid + 256 * h;
      if (h == 0 || second) {
        const int X = ch / kBlocks, Y = ch - X * kBlocks;
        uint32_t* d = img + c * (kStateChunks) + 4 * X * kBlocks + Y;
        d[0] = v[c][h].x;
        d[kBlocks] = v[c][h].y;
        d[2 * kBlocks] = v[c][h].z;
        d[3 * kBlocks] = v[c][h].w;
      }
    }
  }
  __syncthreads();
  uint4* o = reinterpret_cast<uint4*>(out);
  if (LAYOUT == QLX_OBS_NCHW_TIME) {
    const uint4* im = reinterpret_cast<const uint4*>(img);
    for (int i = tid; i < kStateChunks; i += 256) o[i] = im[i];
  } else {
    for (int d = tid; d < kStateChunks; d += 256) {
      const uint32_t w0 = img[d], w1 = img[kStateChunks + d], w2 = img[2 * kStateChunks + d], w3 = img[3 * kStateChunks + d];
      // w_s byte y = pixel y of slot s; output dword y = (w0.y, w1.y, w2.y, w3.y)
      const uint32_t lo01 = byte_perm(w1, w0, 0x05010400u), hi01 = byte_perm(w1, w0, 0x07030602u);
      const uint32_t lo23 = byte_perm(w3, w2, 0x05010400u), hi23 = byte_perm(w3, w2, 0x07030602u);
      o[d] = make_uint4(byte_perm(lo23, lo01, 0x05040100u), byte_perm(lo23, lo01, 0x07060302u),
                        byte_perm(hi23, hi01, 0x05040100u), byte_perm(hi23, hi01, 0x07060302u));
    }
  }
}

// action and n-step window of each sample, one thread per sample (k_replay_nstep's arithmetic: replay_nstep); the window's
// last index also goes to `last_scratch`, where the unpack kernel finds the transition of s'.  Outputs may be null.
__global__ __launch_bounds__(256) void k_batch_meta(ReplayView r, const uint64_t* idx, uint32_t B, uint32_t n_step, float gamma,
                                                    qlx_batch_dev o, uint64_t* last_scratch, uint32_t* flag) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const uint64_t i = idx[b];
  if (i >= r.len) {
    atomicOr(flag, 1u);
    last_scratch[b] = kBadIndex;
    if (o.actions) o.actions[b] = 0;
    if (o.returns) o.returns[b] = 0.0f;
    if (o.discounts) o.discounts[b] = 0.0f;
    if (o.terminals) o.terminals[b] = 1;
    if (o.last_indices) o.last_indices[b] = i;
    if (o.steps) o.steps[b] = 0;
    return;
  }
  const NStepWindow w = replay_nstep(r, i, n_step, gamma);
  last_scratch[b] = w.last_i;
  if (o.actions) o.actions[b] = r.action[(r.total - r.len + i) % r.cap];
  if (o.returns) o.returns[b] = w.R;
  if (o.discounts) o.discounts[b] = w.g;
  if (o.terminals) o.terminals[b] = w.terminal ? 1 : 0;
  if (o.last_indices) o.last_indices[b] = w.last_i;
  if (o.steps) o.steps[b] = w.m;
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <class Source>
static void launch_unpack(int32_t layout, dim3 grid, hipStream_t s, const Source& src) {
  if (layout == QLX_OBS_NCHW_TIME)
    hipLaunchKernelGGL((k_unpack_states<QLX_OBS_NCHW_TIME, Source>), grid, dim3(256), 0, s, src);
  else
    hipLaunchKernelGGL((k_unpack_states<QLX_OBS_NHWC_SLOT, Source>), grid, dim3(256), 0, s, src);
  QLX_HIP(hipGetLastError());
}

// the window scratch and the flag word of the replay's _dev calls: reserved once, at their largest size
static void reserve_dev_scratch(qlx_replay* r) {
  if (r->d_flags) return;
  r->d_win_last.alloc(kMaxBatch);
  r->d_flags.alloc(4);
  QLX_HIP(hipMemsetAsync(r->d_flags, 0, 16, r->stream));
}

}  // namespace qlx

using namespace qlx;

extern "C" {

int32_t qlx_env_stream(qlx_env* e, void** out) {
  return guard([&] {
    QLX_CHECK(e, QLX_E_INVALID, "null env");
    QLX_CHECK(out, QLX_E_INVALID, "null hip_stream_out");
    *out = e->stream;
  });
}

int32_t qlx_replay_stream(qlx_replay* r, void** out) {
  return guard([&] {
    QLX_CHECK(r, QLX_E_INVALID, "null replay");
    QLX_CHECK(out, QLX_E_INVALID, "null hip_stream_out");
    *out = r->stream;
  });
}

int32_t qlx_replay_share_stream(qlx_replay* r, qlx_env* e) {
  return guard([&] {
    QLX_CHECK(r, QLX_E_INVALID, "null replay");
    QLX_CHECK(e, QLX_E_INVALID, "null env");
    QLX_CHECK(r->device == e->device, QLX_E_INVALID, "replay and env are on different devices");
    if (r->stream == e->stream) return;
    QLX_HIP(hipSetDevice(r->device));
    QLX_HIP(hipStreamSynchronize(r->stream));
    adopt_stream(r, e->stream);
  });
}

int32_t qlx_replay_sync(qlx_replay* r) {
  return guard([&] {
    QLX_CHECK(r, QLX_E_INVALID, "null replay");
    QLX_HIP(hipSetDevice(r->device));
    QLX_HIP(hipStreamSynchronize(r->stream));
    if (!r->d_flags) return;
    uint32_t flag = 0;
    QLX_HIP(hipMemcpy(&flag, r->d_flags, 4, hipMemcpyDeviceToHost));
    if (flag) QLX_HIP(hipMemset(r->d_flags, 0, 4));
    QLX_CHECK(flag == 0, QLX_E_INVALID,
              "replay index out of range (>= len) in a device call (or, in a priority write, a td_abs that is NaN, infinite or "
              "negative)");
  });
}

int32_t qlx_env_obs_dev(qlx_env* e, int32_t layout, uint8_t* d_out) {
  return guard([&] {
    QLX_CHECK(e, QLX_E_INVALID, "null env");
    QLX_CHECK(d_out, QLX_E_INVALID, "null d_out");
    QLX_CHECK(layout == QLX_OBS_NHWC_SLOT || layout == QLX_OBS_NCHW_TIME, QLX_E_INVALID, "unknown layout");
    QLX_CHECK(aligned16(d_out), QLX_E_INVALID, "d_out is not 16-byte aligned");
    QLX_HIP(hipSetDevice(e->device));
    const EnvSource src = {e->d_obs, e->d_state, d_out};
    launch_unpack(layout, dim3(e->n), e->stream, src);
  });
}

int32_t qlx_env_reset_dev(qlx_env* e, const uint8_t* d_mask) {
  return guard([&] {
    QLX_CHECK(e, QLX_E_INVALID, "null env");
    QLX_HIP(hipSetDevice(e->device));
    env_launch_reset(e, d_mask, 1);
  });
}

int32_t qlx_replay_sample_distinct_dev(qlx_replay* r, uint64_t seed, uint32_t update_idx, uint32_t rank, uint32_t batch,
                                       uint64_t* d_out) {
  return guard([&] {
    QLX_CHECK(r, QLX_E_INVALID, "null replay");
    QLX_CHECK(d_out, QLX_E_INVALID, "null d_out_indices");
    QLX_CHECK(batch > 0 && batch <= kMaxBatch, QLX_E_INVALID, "batch must be in 1..4096");
    QLX_CHECK(r->len() >= batch, QLX_E_INVALID, "batch: the replay holds fewer transitions (len)");
    QLX_HIP(hipSetDevice(r->device));
    launch_sample_distinct(r->stream, seed, update_idx, 1, rank, r->len(), batch, d_out);
  });
}

int32_t qlx_replay_batch_dev(qlx_replay* r, const uint64_t* d_indices, uint32_t batch, uint32_t n_step, float gamma,
                             int32_t layout, const qlx_batch_dev* out) {
  return guard([&] {
    QLX_CHECK(r, QLX_E_INVALID, "null replay");
    QLX_CHECK(out, QLX_E_INVALID, "null out");
    QLX_CHECK(d_indices, QLX_E_INVALID, "null d_indices");
    QLX_CHECK(layout == QLX_OBS_NHWC_SLOT || layout == QLX_OBS_NCHW_TIME, QLX_E_INVALID, "unknown layout");
    QLX_CHECK(batch > 0 && batch <= kMaxBatch, QLX_E_INVALID, "batch must be in 1..4096");
    QLX_CHECK(n_step >= 1 && n_step <= QLX_NSTEP_MAX, QLX_E_INVALID, "n_step must be in 1..QLX_NSTEP_MAX");
    QLX_CHECK(aligned16(out->s), QLX_E_INVALID, "out->s is not 16-byte aligned");
    QLX_CHECK(aligned16(out->s_next), QLX_E_INVALID, "out->s_next is not 16-byte aligned");
    const qlx_batch_dev o = *out;
    QLX_HIP(hipSetDevice(r->device));
    reserve_dev_scratch(r);
    const ReplayView v = replay_view(r);
    const bool meta = o.s_next || o.actions || o.returns || o.discounts || o.terminals || o.last_indices || o.steps;
    if (meta) {
      hipLaunchKernelGGL(k_batch_meta, dim3((batch + 255) / 256), dim3(256), 0, r->stream, v, d_indices, batch, n_step, gamma, o,
                         r->d_win_last.get(), r->d_flags.get());
      QLX_HIP(hipGetLastError());
    }
    if (o.s || o.s_next) {
      ReplaySource src;
      src.r = v;
      src.idx = d_indices;
      src.last = r->d_win_last;
      src.out[0] = o.s;
      src.out[1] = o.s_next;
      src.which0 = o.s ? 0 : 1;
      src.flag = r->d_flags;
      launch_unpack(layout, dim3(batch, o.s && o.s_next ? 2 : 1), r->stream, src);
    }
  });
}

// ---- prioritized replay on device tensors: the kernels and their launchers are per.hip's ----

int32_t qlx_replay_per_enable(qlx_replay* r) {
  return guard([&] {
    QLX_CHECK(r, QLX_E_INVALID, "null replay");
    QLX_HIP(hipSetDevice(r->device));
    QLX_HIP(hipDeviceSynchronize());   // pushes may be in flight on an env's stream
    reserve_dev_scratch(r);
    PerState& st = r->prio;
    if (!st.d_tree) {
      try {
        st.init(r->cap, 0);
      } catch (...) {   // a failure part-way releases what was built
        st = PerState();
        throw;
      }
    }
    const float one = 1.0f;
    QLX_HIP(hipMemsetAsync(st.d_tree, 0, st.d_tree.bytes(), r->stream));
    QLX_HIP(hipMemsetAsync(st.d_owner, 0, st.d_owner.bytes(), r->stream));
    QLX_HIP(hipMemcpyAsync(st.d_max, &one, sizeof(float), hipMemcpyHostToDevice, r->stream));
    if (r->len()) QLX_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(st.leaves()), (int)f32_bits(one), r->len(), r->stream));
    per_launch_build(r->stream, st.d_tree, st.L);
    QLX_HIP(hipStreamSynchronize(r->stream));
    r->per_on = true;
  });
}

int32_t qlx_replay_per_sample_dev(qlx_replay* r, uint64_t seed, uint32_t update_idx, uint32_t rank, uint32_t batch, float beta,
                                  uint64_t* d_out_indices, float* d_out_weights) {
  return guard([&] {
    QLX_CHECK(r, QLX_E_INVALID, "null replay");
    QLX_CHECK(d_out_indices, QLX_E_INVALID, "null d_out_indices");
    QLX_CHECK(batch > 0 && batch <= kMaxBatch, QLX_E_INVALID, "batch must be in 1..4096");
    QLX_CHECK(std::isfinite(beta) && beta >= 0.0f, QLX_E_INVALID, "beta must be finite and >= 0");
    QLX_CHECK(r->len() > 0, QLX_E_INVALID, "prioritized draw: the replay is empty (len == 0)");
    QLX_CHECK(r->per_on, QLX_E_STATE, "priorities are not enabled (qlx_replay_per_enable)");
    QLX_HIP(hipSetDevice(r->device));
    const uint64_t len = r->len();
    per_launch_draw(r->stream, r->prio.d_tree, r->prio.L, seed, update_idx, rank, len, beta, batch, r->cap,
                    (r->total - len) % r->cap, d_out_indices, d_out_weights);
  });
}

int32_t qlx_replay_per_update_dev(qlx_replay* r, const uint64_t* d_indices, const float* d_td_abs, uint32_t n, float alpha,
                                  float eps) {
  return guard([&] {
    QLX_CHECK(r, QLX_E_INVALID, "null replay");
    QLX_CHECK(n <= kMaxBatch, QLX_E_INVALID, "n must be in 0..4096");
    QLX_CHECK(n == 0 || d_indices, QLX_E_INVALID, "null d_indices");
    QLX_CHECK(n == 0 || d_td_abs, QLX_E_INVALID, "null d_td_abs");
    QLX_CHECK(std::isfinite(alpha) && alpha >= 0.0f, QLX_E_INVALID, "alpha must be finite and >= 0");
    QLX_CHECK(std::isfinite(eps) && eps > 0.0f, QLX_E_INVALID, "eps must be finite and > 0");
    QLX_CHECK(r->per_on, QLX_E_STATE, "priorities are not enabled (qlx_replay_per_enable)");
    if (n == 0) return;
    QLX_HIP(hipSetDevice(r->device));
    PerState& st = r->prio;
    const uint64_t len = r->len(), start = (r->total - len) % r->cap;
    per_launch_update_guarded(r->stream, d_indices, d_td_abs, n, len, r->cap, start, alpha, eps, st.d_owner, st.leaves(), st.d_max,
                              r->d_flags);
    per_launch_build(r->stream, st.d_tree, st.L);   // a refit of the changed paths alone measured no faster
  });
}

int32_t qlx_replay_per_get(qlx_replay* r, float* leaves, float* tree, uint32_t* L, float* total, float* per_max, uint64_t* start) {
  return guard([&] {
    QLX_CHECK(r, QLX_E_INVALID, "null replay");
    QLX_CHECK(r->per_on, QLX_E_STATE, "priorities are not enabled (qlx_replay_per_enable)");
    QLX_HIP(hipSetDevice(r->device));
    QLX_HIP(hipDeviceSynchronize());
    const PerState& st = r->prio;
    if (leaves) QLX_HIP(hipMemcpy(leaves, st.leaves(), r->cap * 4, hipMemcpyDeviceToHost));
    if (tree) QLX_HIP(hipMemcpy(tree, st.d_tree, st.d_tree.bytes(), hipMemcpyDeviceToHost));
    if (L) *L = st.L;
    if (total) QLX_HIP(hipMemcpy(total, st.d_tree + 1, 4, hipMemcpyDeviceToHost));
    if (per_max) QLX_HIP(hipMemcpy(per_max, st.d_max, 4, hipMemcpyDeviceToHost));
    if (start) *start = (r->total - r->len()) % r->cap;
  });
}

}  // extern "C"
