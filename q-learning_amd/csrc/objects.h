// Host-side definitions of the opaque ABI objects (internal).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "per.h"
#include "qlx_internal.h"

struct qlx_env {
  int device = 0;
  uint32_t n = 0;
  uint64_t seed = 0;
  uint32_t id_offset = 0;         // global id of env 0 (data-parallel ranks own disjoint ids)
  hipStream_t stream = nullptr;   // owned unless adopted by a learner
  bool own_stream = true;
  qlx::DeviceBuffer<qlx_breakout_state> d_state;
  qlx::DeviceBuffer<uint32_t> d_ep_steps;  // [n] steps taken in the current episode
  qlx::DeviceBuffer<uint8_t> d_obs;        // [n][4][7056] ring frames, s2d layout
  qlx::DeviceBuffer<uint64_t> d_hash;      // [n] running parity checksum
  qlx::DeviceBuffer<uint32_t> d_flags;     // [4] bad-action flag
  qlx::DeviceBuffer<uint8_t> d_tmp_u8, d_tmp_u8b;   // [n] staging
  qlx::DeviceBuffer<float> d_tmp_f32;      // [n]
  qlx::DeviceBuffer<uint8_t> d_obs_view;   // [n][84][84][4] qlx_env_obs's tensor view (allocated on its first call, kept)
  float acos_thr = 0.0f;
  bool hashing = true;
};

struct qlx_replay {
  int device = 0;
  uint64_t cap = 0;
  uint32_t n = 0;
  uint64_t F = 0;        // frame slots = cap + 4 n
  uint64_t total = 0;    // transitions pushed so far
  hipStream_t stream = nullptr;
  bool own_stream = true;
  qlx::DeviceBuffer<uint8_t> d_frames, d_action, d_done;
  qlx::DeviceBuffer<float> d_reward;
  qlx::DeviceBuffer<uint32_t> d_epstep;
  qlx::DeviceBuffer<uint64_t> d_idx;    // scratch for sampling [max_batch]
  qlx::DeviceBuffer<uint64_t> d_win_last;   // [4096] qlx_replay_batch_dev: each window's last index (reserved at its first call, kept)
  qlx::DeviceBuffer<uint32_t> d_flags;      // [4] sticky bad-index flag of the _dev calls (with d_win_last)
  qlx::PerState prio;                       // priorities of the device-tensor calls (qlx_replay_per_enable)
  bool per_on = false;
  uint64_t len() const { return total < cap ? total : cap; }
};

namespace qlx {
// A learner runs its env, replay and models on its own stream: the object's stream (idle: every create ends synchronised)
// is destroyed, not dropped - a stream holds device memory of its own.
template <class Obj>
void adopt_stream(Obj* o, hipStream_t s) {
  if (o->own_stream) (void)hipStreamDestroy(o->stream);
  o->stream = s;
  o->own_stream = false;
}
// n_updates batches of `batch` distinct logical replay indices < len (replay.hip), for any learner's uniform sampling
void launch_sample_distinct(hipStream_t s, uint64_t seed, uint32_t first_update, uint32_t n_updates, uint32_t rank, uint64_t len,
                            uint32_t batch, uint64_t* d_out);

// Reads the Keras SavedModel variables of `n_layers` weight layers (kernel, bias, Adam m / v) from a TF bundle
// into host arrays laid out like the flat parameter vector (variable 2L = kernel L, 2L + 1 = bias L) and the
// optimizer iteration count.  Shapes must multiply to var_sizes.  (tf_bundle.cpp)
void load_keras_bundle(const char* prefix, int n_layers, const int* var_sizes, std::vector<float>& w, std::vector<float>& m,
                       std::vector<float>& v, int64_t* iterations);

void env_launch_step(qlx_env* env, const uint8_t* d_actions, float* d_rewards, uint8_t* d_dones);
void env_launch_reset(qlx_env* env, const uint8_t* d_mask, int bump);
void replay_launch_push(qlx_replay* rb, qlx_env* env, hipStream_t s, const uint8_t* d_actions, const float* d_rewards,
                        const uint8_t* d_dones);
}  // namespace qlx
