// The wide output head: a dense layer 512 -> width on a4 of one fp32 qlx_model, attached beside the
// model's ten variables.  The object and its layout; kernels and entry points are in head_wide.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "qlx_internal.h"

struct qlx_model;

namespace qlx {
constexpr int kHeadIn = 512;          // a4 features
constexpr uint32_t kHeadInitVar = 10; // Wh's init stream: (seed, 10, 0, P_INIT) - the variable index after the model's ten
}  // namespace qlx

struct qlx_head {
  qlx_model* model = nullptr;
  int width = 0;
  // Wh [512][width] then bh [width], the same layout in every buffer; count = 513 * width
  qlx::DeviceBuffer<float> d_w, d_m, d_v, d_grads;
  qlx::DeviceBuffer<float> d_part;   // clip-norm scratch: Wh's segment partials, then bh's one, then the two norms
  qlx::DeviceBuffer<float> d_zero;   // [4096][3] zeros: the fc1 backward's dq when the caller gives none
  qlx::DeviceBuffer<float> d_dist;   // [4096] per-sample losses of a distributional loss whose caller wants none (§20)
  int64_t iterations = 0;
  hipEvent_t event = nullptr;        // orders qlx_head_copy_weights_dev across two streams (created at its first use)
  int64_t count() const { return (int64_t)(qlx::kHeadIn + 1) * width; }
  int64_t bias_offset() const { return (int64_t)qlx::kHeadIn * width; }
};

namespace qlx {
// Z [n][width] = a4 Wh + bh of the model's last trunk forward over n rows: the one k_headw_fwd launch, with the grid choice
// every caller shares (qlx_head_forward_dev, the evaluator's head run), so the bits are the same whoever asks
void head_forward_launch(qlx_head* h, uint32_t n, float* d_z, hipStream_t s);
}  // namespace qlx
