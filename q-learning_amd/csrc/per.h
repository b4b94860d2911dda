// Prioritized replay state and launchers (per.hip), shared by the learner and the standalone qlx_sumtree.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "device_memory.h"

namespace qlx {

struct PerState {
  uint64_t cap = 0;
  uint32_t L = 0;               // leaves (power of two >= cap); node i of the heap at d_tree[i], leaves at d_tree + L
  DeviceBuffer<float> d_tree;      // [2L]
  DeviceBuffer<uint32_t> d_owner;  // [L] last-writer claims of the priority write (zero between launches)
  DeviceBuffer<float> d_max;       // largest priority so far (new transitions enter with it), starts at 1
  DeviceBuffer<float> d_w;         // [max samples] IS weights of the sampled batches
  DeviceBuffer<float> d_td;        // [max samples] |TD error| of the sampled transitions
  void init(uint64_t capacity, size_t max_samples);
  float* leaves() const { return d_tree + L; }
};

uint32_t per_leaves(uint64_t cap);
void per_launch_build(hipStream_t s, float* tree, uint32_t L);
// n_updates batches of B draws; out: logical replay indices ((slot - start) mod cap) and normalised IS weights
void per_launch_sample(hipStream_t s, const float* tree, uint32_t L, uint64_t seed, uint32_t first_update, uint32_t n_updates,
                       uint32_t rank, uint64_t len, float beta, uint32_t B, uint64_t cap, uint64_t start, uint64_t* idx_out,
                       float* w_out);
void per_launch_push(hipStream_t s, float* leaves, uint64_t cap, uint64_t first, uint32_t n, const float* per_max);
void per_launch_update(hipStream_t s, const uint64_t* idx, const float* td_abs, uint32_t n, uint64_t cap, uint64_t start,
                       float alpha, float eps, uint32_t* owner, float* leaves, float* per_max);

// ---- one batch per call (the replay's device-tensor calls) ----
// B <= 4096 draws of update `update_idx` from a built tree: k_per_sample's draws bit for bit; w_out may be null
void per_launch_draw(hipStream_t s, const float* tree, uint32_t L, uint64_t seed, uint32_t update_idx, uint32_t rank, uint64_t len,
                     float beta, uint32_t B, uint64_t cap, uint64_t start, uint64_t* idx_out, float* w_out);
// per_launch_update with the data the host cannot see guarded: an index >= len or a td_abs that is NaN, infinite or
// negative writes nothing and sets *flag
void per_launch_update_guarded(hipStream_t s, const uint64_t* idx, const float* td_abs, uint32_t n, uint64_t len, uint64_t cap,
                               uint64_t start, float alpha, float eps, uint32_t* owner, float* leaves, float* per_max,
                               uint32_t* flag);

}  // namespace qlx
