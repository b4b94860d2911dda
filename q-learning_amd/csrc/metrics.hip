// Per-update training metrics: k_update_metrics reduces the Q values the training head wrote, the batch's actions,
// targets and IS weights, the loss and Adam's pre-clip gradient norms into one qlx_update_metrics row (include/qlx.h).
// Beyond the reference (its nearest interface is learning_update_log, self_driving_tf_q_learner.rs:235-273).
//
// Reduction order (every field is bit-reproducible): thread t of 256 takes samples t, t + 256, .. in ascending order and
// adds each mean's terms to a double; the 64 partials of a wave meet in an xor butterfly (offsets 32, 16, .. 1: every
// lane ends with the same sum, fp addition being commutative); the four wave partials are added in wave order,
// ((w0 + w1) + w2) + w3, divided by B and rounded to float once.  Minima and maxima are order-independent; the counts and
// the histogram are integer LDS atomics, order-independent too.  No float atomics, one workgroup, no data between
// workgroups.
#include "metrics.h"

namespace qlx {

namespace {

constexpr int kSums = 6;   // q_taken, q_max, action_gap, y, td_abs, weight
constexpr int kExts = 5;   // q_taken min / max, y min / max, td_abs max
// LDS counters: argmax_counts [8], td_hist [16], n_linear, n_nonfinite
constexpr int kCntArgmax = 0, kCntHist = 8, kCntLinear = 24, kCntNonfinite = 25, kCnts = 26;

__device__ inline bool finite_f32(float x) { return (f32_bits(x) & 0x7F800000u) != 0x7F800000u; }

}  // namespace

__global__ __launch_bounds__(256) void k_update_metrics(MetricsArgs A) {
  __shared__ uint32_t s_cnt[kCnts];
  __shared__ double s_sum[4][kSums];
  __shared__ float s_ext[4][kExts];
  __shared__ float s_norm[kMetricsMaxVars];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < kCnts) s_cnt[tid] = 0;
  __syncthreads();
  const float inf = __builtin_huge_valf();
  double sum[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  float qa_min = inf, qa_max = -inf, y_min = inf, y_max = -inf, td_max = 0.0f;
  uint32_t n_linear = 0, n_nonfinite = 0;
  // the update's norms and loss are loaded first, so their latency hides behind the sample loop
  const float my_norm = (uint32_t)tid < A.n_vars ? A.norms[tid] : 0.0f;
  const float loss = tid == 0 ? A.loss[0] : 0.0f;
  // a thread's samples four at a time: the loads of all four are in flight together, then they are consumed in
  // ascending order (the summation order is that of one sample at a time)
  for (uint32_t b0 = (uint32_t)tid; b0 < A.B; b0 += 4 * 256) {
    float qv[4][kMetricsMaxActions], yv[4], wv[4];
    uint32_t av[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t b = b0 + 256u * j < A.B ? b0 + 256u * j : b0;   // past the batch: a valid sample, not consumed
      const float* qb = A.q + (size_t)b * A.n_actions;
#pragma unroll
      for (uint32_t k = 0; k < kMetricsMaxActions; ++k) qv[j][k] = k < A.n_actions ? qb[k] : -inf;
      av[j] = A.actions[b];
      yv[j] = A.y[b];
      wv[j] = A.weights ? A.weights[b] : 1.0f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (b0 + 256u * j >= A.B) break;
      uint32_t best = 0;   // tf.argmax: first maximal index
      float top = qv[j][0];
#pragma unroll
      for (uint32_t k = 1; k < kMetricsMaxActions; ++k)
        if (k < A.n_actions && qv[j][k] > top) { best = k; top = qv[j][k]; }
      float second = -inf;
#pragma unroll
      for (uint32_t k = 0; k < kMetricsMaxActions; ++k)
        if (k < A.n_actions && k != best) second = fmaxf(second, qv[j][k]);
      const uint32_t act = av[j] < A.n_actions ? av[j] : A.n_actions - 1;
      float qa = qv[j][0];
#pragma unroll
      for (uint32_t k = 1; k < kMetricsMaxActions; ++k)
        if (k == act) qa = qv[j][k];
      const float y = yv[j];
      const float td = fabsf(__fsub_rn(qa, y));
      sum[0] += (double)qa;
      sum[1] += (double)top;
      sum[2] += (double)__fsub_rn(top, second);
      sum[3] += (double)y;
      sum[4] += (double)td;
      sum[5] += (double)wv[j];
      qa_min = fminf(qa_min, qa);
      qa_max = fmaxf(qa_max, qa);
      y_min = fminf(y_min, y);
      y_max = fmaxf(y_max, y);
      td_max = fmaxf(td_max, td);
      n_linear += td > 1.0f ? 1u : 0u;
      n_nonfinite += finite_f32(qa) && finite_f32(y) ? 0u : 1u;
      atomicAdd(&s_cnt[kCntArgmax + best], 1u);
      atomicAdd(&s_cnt[kCntHist + metrics_td_bin(td)], 1u);
    }
  }
  if (n_linear) atomicAdd(&s_cnt[kCntLinear], n_linear);
  if (n_nonfinite) atomicAdd(&s_cnt[kCntNonfinite], n_nonfinite);
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int k = 0; k < kSums; ++k) sum[k] += __shfl_xor(sum[k], off);
    qa_min = fminf(qa_min, __shfl_xor(qa_min, off));
    qa_max = fmaxf(qa_max, __shfl_xor(qa_max, off));
    y_min = fminf(y_min, __shfl_xor(y_min, off));
    y_max = fmaxf(y_max, __shfl_xor(y_max, off));
    td_max = fmaxf(td_max, __shfl_xor(td_max, off));
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kSums; ++k) s_sum[wave][k] = sum[k];
    s_ext[wave][0] = qa_min;
    s_ext[wave][1] = qa_max;
    s_ext[wave][2] = y_min;
    s_ext[wave][3] = y_max;
    s_ext[wave][4] = td_max;
  }
  if (tid < (int)kMetricsMaxVars) s_norm[tid] = my_norm;
  __syncthreads();
  qlx_update_metrics* r = A.row;
  if (tid < (int)kMetricsMaxActions) r->argmax_counts[tid] = s_cnt[kCntArgmax + tid];
  if (tid < 16) r->td_hist[tid] = s_cnt[kCntHist + tid];
  if (tid < (int)kMetricsMaxVars) r->grad_norm[tid] = my_norm;
  if (tid != 0) return;
  float mean[kSums];
#pragma unroll
  for (int k = 0; k < kSums; ++k)
    mean[k] = (float)((((s_sum[0][k] + s_sum[1][k]) + s_sum[2][k]) + s_sum[3][k]) / (double)A.B);
  double g2 = 0.0;
  uint32_t n_clipped = 0;
  for (uint32_t v = 0; v < A.n_vars; ++v) {
    const float nv = s_norm[v];
    g2 += (double)nv * (double)nv;
    n_clipped += nv > A.clipnorm ? 1u : 0u;
  }
  r->update = A.update;
  r->step_count = A.step_count;
  r->batch = A.B;
  r->n_actions = A.n_actions;
  r->n_vars = A.n_vars;
  r->n_clipped = n_clipped;
  r->n_linear = s_cnt[kCntLinear];
  r->n_nonfinite = s_cnt[kCntNonfinite];
  r->loss = loss;
  r->q_taken_mean = mean[0];
  r->q_taken_min = fminf(fminf(s_ext[0][0], s_ext[1][0]), fminf(s_ext[2][0], s_ext[3][0]));
  r->q_taken_max = fmaxf(fmaxf(s_ext[0][1], s_ext[1][1]), fmaxf(s_ext[2][1], s_ext[3][1]));
  r->q_max_mean = mean[1];
  r->action_gap_mean = mean[2];
  r->y_mean = mean[3];
  r->y_min = fminf(fminf(s_ext[0][2], s_ext[1][2]), fminf(s_ext[2][2], s_ext[3][2]));
  r->y_max = fmaxf(fmaxf(s_ext[0][3], s_ext[1][3]), fmaxf(s_ext[2][3], s_ext[3][3]));
  r->td_abs_mean = mean[4];
  r->td_abs_max = fmaxf(fmaxf(s_ext[0][4], s_ext[1][4]), fmaxf(s_ext[2][4], s_ext[3][4]));
  r->weight_mean = mean[5];
  r->grad_norm_global = (float)sqrt(g2);
  r->reserved = 0;
}

void launch_update_metrics(hipStream_t s, const MetricsArgs& a) {
  QLX_CHECK(a.B >= 1 && a.n_actions >= 2 && a.n_actions <= kMetricsMaxActions && a.n_vars <= kMetricsMaxVars, QLX_E_INVALID,
            "update metrics: batch, n_actions or n_vars out of range");
  hipLaunchKernelGGL(k_update_metrics, dim3(1), dim3(256), 0, s, a);
  QLX_HIP(hipGetLastError());
}

}  // namespace qlx

extern "C" int32_t qlx_metrics_td_bin(float td_abs) { return qlx::metrics_td_bin(td_abs); }
