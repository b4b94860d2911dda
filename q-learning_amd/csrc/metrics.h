// Per-update training metrics (metrics.hip): one kernel per update reduces what the update left in device memory into a
// qlx_update_metrics row of a ring; LearnerCore::record_metrics launches it, the host drains the ring (DESIGN.md
// "Training metrics").
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "qlx_internal.h"

namespace qlx {

constexpr uint32_t kMetricsMaxActions = 8;    // qlx_update_metrics.argmax_counts
constexpr uint32_t kMetricsMaxVars = 16;      // qlx_update_metrics.grad_norm
constexpr uint32_t kMetricsMaxRows = 1u << 20;

// td_hist bin of |td| from its exponent bits: biased exponent 116 is 2^-11, the lower edge of bin 1; 130 is 8 = 2^3, the
// lower edge of bin 15 (255, inf and NaN, lands there too); below 116 (0 and denormals included) is bin 0
__host__ __device__ inline int metrics_td_bin(float td_abs) {
  const int k = (int)((f32_bits(td_abs) & 0x7FFFFFFFu) >> 23) - 115;
  return k < 0 ? 0 : (k > 15 ? 15 : k);
}

struct MetricsArgs {
  const float* q;           // [B][n_actions] as the training head wrote it
  const uint8_t* actions;   // [B]
  const float* y;           // [B]
  const float* weights;     // [B] IS weights, or null (weight_mean = 1)
  const float* loss;        // the update's loss
  const float* norms;       // [n_vars] pre-clip gradient norms after the update's Adam
  uint32_t B, n_actions, n_vars;
  float clipnorm;
  uint64_t update, step_count;
  qlx_update_metrics* row;
};

// one workgroup of 256 threads on `s`; B >= 1, n_actions in 2 .. kMetricsMaxActions, n_vars <= kMetricsMaxVars
void launch_update_metrics(hipStream_t s, const MetricsArgs& a);

}  // namespace qlx
