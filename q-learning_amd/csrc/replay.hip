// HBM-resident replay ring with on-GPU distinct sampling (gfx950).
//
// Reference behaviour (restated): ReplayBuffer::add / get_many (replay_buffer.rs:21-38, 85-98, 126-137),
// generate_distinct_random_ids (self_driving_tf_q_learner.rs:276-296) with rand 0.8.5's
// Uniform<usize> zone rejection.  Layout and state reconstruction: replay_dev.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "objects.h"
#include "replay_dev.h"

namespace qlx {

// push: one workgroup (256 threads) per env copies the env's newest frame (28 x 16 B per thread-pass)
// and thread 0 writes the transition metadata.
__global__ __launch_bounds__(256) void k_replay_push(const uint8_t* obs, const qlx_breakout_state* st,
                                                     const uint32_t* ep_steps, uint32_t n, const uint8_t* actions,
                                                     const float* rewards, const uint8_t* dones, uint8_t* frames,
                                                     uint8_t* r_action, float* r_reward, uint8_t* r_done,
                                                     uint32_t* r_epstep, uint64_t total, uint64_t cap, uint64_t F) {
  const uint32_t e = blockIdx.x;
  const uint64_t p = total + e;
  const int slot = (st[e].next_slot + 3) & 3;
  const uint4* src = reinterpret_cast<const uint4*>(obs + ((size_t)e * kSlots + slot) * kFramePix);
  uint4* dst = reinterpret_cast<uint4*>(frames + (p % F) * kFramePix);
  for (int i = threadIdx.x; i < kFramePix / 16; i += blockDim.x) dst[i] = src[i];
  if (threadIdx.x == 0) {
    const uint64_t t = p % cap;
    r_action[t] = actions[e];
    r_reward[t] = rewards[e];
    r_done[t] = dones[e];
    r_epstep[t] = ep_steps[e];
  }
}

__device__ __forceinline__ uint64_t umulhi64(uint64_t a, uint64_t b, uint64_t* lo) {
  const unsigned __int128 m = (unsigned __int128)a * b;
  *lo = (uint64_t)m;
  return (uint64_t)(m >> 64);
}

// generate_distinct_random_ids, one 256-thread block per update.  256 consecutive u64 draws are evaluated in
// parallel per round; a draw is kept iff it passes the zone test and no earlier draw (an earlier round's keep,
// or an earlier draw of this round) has the same value - the sequential loop's result.  Every accepted draw
// claims its value's slot of an LDS hash set (keys u32: values < len < 2^32 - 1) and atomicMin's its draw
// index into the slot's owner word; after a barrier a draw is kept iff it owns its slot (an earlier round's
// keep owns it with a smaller index).  Kept draws are compacted in draw order by a block prefix count.
constexpr int kSampleThreads = 256;
__global__ __launch_bounds__(kSampleThreads) void k_sample_distinct(uint64_t seed, uint32_t first_update, uint32_t rank,
                                                                    uint64_t len, uint32_t B, uint32_t log2_table,
                                                                    uint64_t* out) {
  extern __shared__ uint32_t sh[];
  const uint32_t tsize = 1u << log2_table;
  uint32_t* keys = sh;
  uint32_t* owner = sh + tsize;
  __shared__ uint32_t wave_cnt[kSampleThreads / 64];
  const uint32_t u = first_update + blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t EMPTY = 0xFFFFFFFFu;
  for (uint32_t i = tid; i < tsize; i += kSampleThreads) { keys[i] = EMPTY; owner[i] = EMPTY; }
  __syncthreads();
  const uint64_t zone = ~0ull - ((~0ull - len + 1) % len);
  uint64_t* dst = out + (size_t)blockIdx.x * B;
  uint32_t count = 0;
  for (uint64_t round = 0; count < B; ++round) {
    const uint64_t d = round * kSampleThreads + tid;
    RngStream rs(seed, u, rank, P_SAMPLE, 2 * d);
    const uint64_t v = rs.u64();
    uint64_t lo;
    const uint32_t hi = (uint32_t)umulhi64(v, len, &lo);
    const bool acc = lo <= zone;
    uint32_t h = 0;
    if (acc) {
      h = (uint32_t)(((uint64_t)hi * 0x9E3779B97F4A7C15ull) >> (64 - log2_table));
      for (;;) {
        const uint32_t t = atomicCAS(&keys[h], EMPTY, hi);
        if (t == EMPTY || t == hi) break;
        h = (h + 1) & (tsize - 1);
      }
      atomicMin(&owner[h], (uint32_t)d);
    }
    __syncthreads();
    const bool ok = acc && owner[h] == (uint32_t)d;
    const unsigned long long bal = __ballot(ok);
    if (lane == 0) wave_cnt[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kSampleThreads / 64; ++w) {
      before += w < wave ? wave_cnt[w] : 0u;
      total += wave_cnt[w];
    }
    const uint32_t pos = count + before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
    if (ok && pos < B) dst[pos] = hi;
    count = min(B, count + total);
    __syncthreads();   // wave_cnt / owner reads done before the next round writes them
  }
}

// get_many + batch_to_multi_dim_array: out [B][84][84][4] (x, y, slot)
__global__ void k_replay_view(ReplayView r, const uint64_t* idx, uint32_t B, int which, uint8_t* out) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (size_t)B * kFramePix) return;
  const uint32_t b = (uint32_t)(g / kFramePix);
  const int xy = (int)(g - (size_t)b * kFramePix);
  const int x = xy / kFrame, y = xy - x * kFrame;
  const uint8_t* f[4];
  replay_frames(r, idx[b], which, f);
  const int off = s2d_offset(x, y);
  uchar4 v;
  v.x = f[0] ? f[0][off] : 0;
  v.y = f[1] ? f[1][off] : 0;
  v.z = f[2] ? f[2][off] : 0;
  v.w = f[3] ? f[3][off] : 0;
  reinterpret_cast<uchar4*>(out)[g] = v;
}

__global__ void k_replay_meta(ReplayView r, const uint64_t* idx, uint32_t B, uint8_t* a, float* rw, uint8_t* d) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const uint64_t t = (r.total - r.len + idx[b]) % r.cap;
  a[b] = r.action[t];
  rw[b] = r.reward[t];
  d[b] = r.done[t];
}

// n-step windows of a list of logical indices (replay_dev.h replay_nstep), one thread per sample; outputs may be null
__global__ __launch_bounds__(256) void k_replay_nstep(ReplayView r, const uint64_t* idx, uint32_t B, uint32_t n_step, float gamma,
                                                      float* ret, float* disc, uint64_t* last, uint8_t* term, uint32_t* steps) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const NStepWindow w = replay_nstep(r, idx[b], n_step, gamma);
  if (ret) ret[b] = w.R;
  if (disc) disc[b] = w.g;
  if (last) last[b] = w.last_i;
  if (term) term[b] = w.terminal ? 1 : 0;
  if (steps) steps[b] = w.m;
}

ReplayView replay_view(const qlx_replay* rb) {
  ReplayView v;
  v.frames = rb->d_frames; v.action = rb->d_action; v.reward = rb->d_reward; v.done = rb->d_done;
  v.epstep = rb->d_epstep; v.cap = rb->cap; v.F = rb->F; v.total = rb->total; v.len = rb->len(); v.n = rb->n;
  return v;
}

void replay_launch_push(qlx_replay* rb, qlx_env* env, hipStream_t s, const uint8_t* d_actions, const float* d_rewards,
                        const uint8_t* d_dones) {
  hipLaunchKernelGGL(k_replay_push, dim3(env->n), dim3(256), 0, s, env->d_obs, env->d_state, env->d_ep_steps, env->n,
                     d_actions, d_rewards, d_dones, rb->d_frames, rb->d_action, rb->d_reward, rb->d_done, rb->d_epstep,
                     rb->total, rb->cap, rb->F);
  QLX_HIP(hipGetLastError());
  if (rb->per_on) {   // priorities enabled (qlx_replay_per_enable): the pushed slots enter at per_max, the tree follows
    per_launch_push(s, rb->prio.leaves(), rb->cap, rb->total, env->n, rb->prio.d_max);
    per_launch_build(s, rb->prio.d_tree, rb->prio.L);
  }
  rb->total += env->n;
}

// the set holds at most B + 255 keys (the last round may claim slots past B): keep it at most half full
static uint32_t table_log2(uint32_t batch) {
  uint32_t l = 8;
  while ((1u << l) < 2 * (batch + kSampleThreads)) ++l;
  return l;
}

void launch_sample_distinct(hipStream_t s, uint64_t seed, uint32_t first_update, uint32_t n_updates, uint32_t rank, uint64_t len,
                            uint32_t batch, uint64_t* d_out) {
  const uint32_t l2 = table_log2(batch);
  QLX_CHECK(len < 0xFFFFFFFFull, QLX_E_INVALID, "replay sampling keys are 32-bit: len must be < 2^32 - 1");
  QLX_CHECK(len >= batch, QLX_E_INVALID, "cannot draw more distinct indices than the replay holds");
  set_lds_limit((const void*)k_sample_distinct, 128 * 1024);   // up to 128 KB of hash set at B = 4096
  hipLaunchKernelGGL(k_sample_distinct, dim3(n_updates), dim3(kSampleThreads), (size_t)8 << l2, s, seed, first_update, rank, len,
                     batch, l2, d_out);
  QLX_HIP(hipGetLastError());
}

}  // namespace qlx

using namespace qlx;

extern "C" {

int32_t qlx_replay_create(uint64_t capacity, uint32_t n_envs, int32_t device, qlx_replay** out) {
  return guard([&] {
    QLX_CHECK(capacity > 0 && n_envs > 0 && out, QLX_E_INVALID, "capacity and n_envs must be > 0");
    current_device_checked(device);
    auto* r = new qlx_replay;
    try {   // a failure part-way releases what was built
      r->device = device;
      r->cap = capacity;
      r->n = n_envs;
      r->F = capacity + 4ull * n_envs;
      QLX_HIP(hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking));
      r->d_frames.alloc(r->F * kFramePix);
      r->d_action.alloc(capacity);
      r->d_reward.alloc(capacity);
      r->d_done.alloc(capacity);
      r->d_epstep.alloc(capacity);
    } catch (...) {
      qlx_replay_destroy(r);
      throw;
    }
    *out = r;
  });
}

int32_t qlx_replay_destroy(qlx_replay* r) {
  return guard([&] {
    if (!r) return;
    (void)hipSetDevice(r->device);
    (void)hipStreamSynchronize(r->stream);
    if (r->own_stream) (void)hipStreamDestroy(r->stream);
    delete r;
  });
}

uint64_t qlx_replay_len(const qlx_replay* r) { return r ? r->len() : 0; }

int32_t qlx_replay_push_dev(qlx_replay* r, qlx_env* env, const uint8_t* d_actions, const float* d_rewards,
                            const uint8_t* d_dones) {
  return guard([&] {
    QLX_CHECK(r && env && d_actions && d_rewards && d_dones, QLX_E_INVALID, "null argument");
    QLX_CHECK(env->n == r->n, QLX_E_INVALID, "replay n_envs differs from env");
    QLX_HIP(hipSetDevice(r->device));
    replay_launch_push(r, env, env->stream, d_actions, d_rewards, d_dones);
  });
}

int32_t qlx_replay_push(qlx_replay* r, qlx_env* env, const uint8_t* actions, const float* rewards,
                        const uint8_t* dones) {
  return guard([&] {
    QLX_CHECK(r && env && actions && rewards && dones, QLX_E_INVALID, "null argument");
    QLX_CHECK(env->n == r->n, QLX_E_INVALID, "replay n_envs differs from env");
    QLX_HIP(hipSetDevice(r->device));
    QLX_HIP(hipMemcpyAsync(env->d_tmp_u8, actions, env->n, hipMemcpyHostToDevice, env->stream));
    QLX_HIP(hipMemcpyAsync(env->d_tmp_f32, rewards, env->n * sizeof(float), hipMemcpyHostToDevice, env->stream));
    QLX_HIP(hipMemcpyAsync(env->d_tmp_u8b, dones, env->n, hipMemcpyHostToDevice, env->stream));
    replay_launch_push(r, env, env->stream, env->d_tmp_u8, env->d_tmp_f32, env->d_tmp_u8b);
    QLX_HIP(hipStreamSynchronize(env->stream));
  });
}

int32_t qlx_replay_sample_distinct(qlx_replay* r, uint64_t seed, uint32_t update_idx, uint32_t rank, uint32_t batch,
                                   uint64_t* out) {
  return guard([&] {
    QLX_CHECK(r && out, QLX_E_INVALID, "null argument");
    QLX_CHECK(batch > 0 && batch <= 4096, QLX_E_INVALID, "batch must be in 1..4096");
    QLX_CHECK(r->len() >= batch, QLX_E_INVALID, "replay holds fewer transitions than the batch");
    QLX_HIP(hipSetDevice(r->device));
    QLX_HIP(hipDeviceSynchronize());
    r->d_idx.reserve(batch);
    launch_sample_distinct(r->stream, seed, update_idx, 1, rank, r->len(), batch, r->d_idx);
    QLX_HIP(hipMemcpyAsync(out, r->d_idx, batch * sizeof(uint64_t), hipMemcpyDeviceToHost, r->stream));
    QLX_HIP(hipStreamSynchronize(r->stream));
  });
}

int32_t qlx_replay_get_many(qlx_replay* r, const uint64_t* indices, uint32_t B, uint8_t* s, uint8_t* s_next,
                            uint8_t* actions, float* rewards, uint8_t* dones) {
  return guard([&] {
    QLX_CHECK(r && indices && B > 0, QLX_E_INVALID, "null argument");
    for (uint32_t b = 0; b < B; ++b) QLX_CHECK(indices[b] < r->len(), QLX_E_INVALID, "index out of range");
    QLX_HIP(hipSetDevice(r->device));
    QLX_HIP(hipDeviceSynchronize());
    const size_t bytes = (size_t)B * kFramePix * kSlots;
    DeviceBuffer<uint64_t> d_idx(B);
    DeviceBuffer<uint8_t> d_out(bytes), d_a(B), d_d(B);
    DeviceBuffer<float> d_r(B);
    QLX_HIP(hipMemcpyAsync(d_idx, indices, B * sizeof(uint64_t), hipMemcpyHostToDevice, r->stream));
    const ReplayView v = replay_view(r);
    const size_t total = (size_t)B * kFramePix;
    for (int which = 0; which < 2; ++which) {
      uint8_t* dst = which ? s_next : s;
      if (!dst) continue;
      hipLaunchKernelGGL(k_replay_view, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, r->stream, v, d_idx, B, which, d_out);
      QLX_HIP(hipGetLastError());
      QLX_HIP(hipMemcpyAsync(dst, d_out, bytes, hipMemcpyDeviceToHost, r->stream));
      QLX_HIP(hipStreamSynchronize(r->stream));
    }
    hipLaunchKernelGGL(k_replay_meta, dim3((B + 255) / 256), dim3(256), 0, r->stream, v, d_idx, B, d_a, d_r, d_d);
    QLX_HIP(hipGetLastError());
    if (actions) QLX_HIP(hipMemcpyAsync(actions, d_a, B, hipMemcpyDeviceToHost, r->stream));
    if (rewards) QLX_HIP(hipMemcpyAsync(rewards, d_r, B * sizeof(float), hipMemcpyDeviceToHost, r->stream));
    if (dones) QLX_HIP(hipMemcpyAsync(dones, d_d, B, hipMemcpyDeviceToHost, r->stream));
    QLX_HIP(hipStreamSynchronize(r->stream));
  });
}

int32_t qlx_replay_nstep(qlx_replay* r, const uint64_t* indices, uint32_t B, uint32_t n_step, float gamma, float* returns,
                         float* discounts, uint64_t* last_indices, uint8_t* terminals, uint32_t* steps) {
  return guard([&] {
    QLX_CHECK(r && indices && B > 0, QLX_E_INVALID, "null argument");
    QLX_CHECK(n_step >= 1 && n_step <= QLX_NSTEP_MAX, QLX_E_INVALID, "n_step must be in 1..QLX_NSTEP_MAX");
    for (uint32_t b = 0; b < B; ++b) QLX_CHECK(indices[b] < r->len(), QLX_E_INVALID, "index out of range");
    QLX_HIP(hipSetDevice(r->device));
    QLX_HIP(hipDeviceSynchronize());
    DeviceBuffer<uint64_t> d_idx(B), d_last(B);
    DeviceBuffer<float> d_ret(B), d_disc(B);
    DeviceBuffer<uint32_t> d_steps(B);
    DeviceBuffer<uint8_t> d_term(B);
    QLX_HIP(hipMemcpyAsync(d_idx, indices, B * sizeof(uint64_t), hipMemcpyHostToDevice, r->stream));
    hipLaunchKernelGGL(k_replay_nstep, dim3((B + 255) / 256), dim3(256), 0, r->stream, replay_view(r), d_idx, B, n_step, gamma,
                       d_ret, d_disc, d_last, d_term, d_steps);
    QLX_HIP(hipGetLastError());
    if (returns) QLX_HIP(hipMemcpyAsync(returns, d_ret, B * sizeof(float), hipMemcpyDeviceToHost, r->stream));
    if (discounts) QLX_HIP(hipMemcpyAsync(discounts, d_disc, B * sizeof(float), hipMemcpyDeviceToHost, r->stream));
    if (last_indices) QLX_HIP(hipMemcpyAsync(last_indices, d_last, B * sizeof(uint64_t), hipMemcpyDeviceToHost, r->stream));
    if (terminals) QLX_HIP(hipMemcpyAsync(terminals, d_term, B, hipMemcpyDeviceToHost, r->stream));
    if (steps) QLX_HIP(hipMemcpyAsync(steps, d_steps, B * sizeof(uint32_t), hipMemcpyDeviceToHost, r->stream));
    QLX_HIP(hipStreamSynchronize(r->stream));
  });
}

}  // extern "C"
