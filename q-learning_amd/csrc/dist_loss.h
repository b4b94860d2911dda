// Distributional losses on the wide head: the kernels' launchers.  Entry points are in dist_loss.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "qlx_internal.h"

namespace qlx {

constexpr uint32_t kDistMaxAtoms = QLX_DIST_MAX_ATOMS;   // 3 * 341 = 1023 <= QLX_HEAD_MAX_WIDTH

// Q [n][3], first argmax and max-Q of n rows z [n][3 N]; any output may be null
void dist_values(const qlx_dist& d, const float* z, uint32_t n, float* q, uint8_t* actions, float* max_q, hipStream_t s);
// the evaluator's rows of a select: row r is env list[r], valid while r < count[1] and kdone[list[r]] < K; counts [3] integer
struct DistSelectRows {
  const uint32_t* list;
  const uint32_t* count;
  const uint32_t* kdone;
  uint32_t K;
  unsigned long long* counts;
};
// values, first argmax and the epsilon-greedy draw of `rows` rows z [rows][3 N] in one launch: row r belongs
// to e = active->list[r] (active null: e = r, every row valid) and draws from the streams (seed, e, t, purpose, words 0 and
// 2); actions [e], qmax [e] (greedy max-Q, may be null), q [r][3] (greedy values, may be null)
void dist_select(const qlx_dist& d, const float* z, uint32_t rows, const DistSelectRows* active, double epsilon, uint64_t seed,
                 uint32_t t, uint32_t purpose, uint8_t* actions, float* qmax, float* q, hipStream_t s);
// every qlx_dist error that can be judged without reading a handle (QLX_E_INVALID naming the field)
void dist_check(const qlx_dist* d);
// a*, target, L_b (sample_loss [B], never null: the head's scratch when the caller wants none) and the whole dz row in one
// launch; the scalar loss, unless null, in a second one-wave launch.  flag: the model's sticky flag word
void dist_loss(const qlx_dist& d, const float* z, const qlx_dist_batch& b, uint32_t B, float* dz, float* loss, float* sample_loss,
               uint8_t* a_star_out, uint32_t* flag, hipStream_t s);

}  // namespace qlx
