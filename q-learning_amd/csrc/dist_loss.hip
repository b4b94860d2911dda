// Distributional losses on the wide head (gfx950): a head of width 3 N read as Z[b][a N + i], with QR-DQN's
// quantile Huber loss (Dabney et al. 2018) and C51's projected cross-entropy (Bellemare et al. 2017) as fused kernels, so an
// update is one enqueue-only call as the built-in Huber head's is.
//
// These kernels are latency-bound at a DQN agent's sizes (B = 1024, N = 51: 2.7 M pair terms, 1.3 MB moved); what they
// remove is a dozen small launches and the host's waits between them, not arithmetic.
//
// Layout of the work.  Loss kernels: one block per sample, 64 ceil(min(N, 256) / 64) threads, thread t owns the rows
// i = t and t + blockDim (N <= 341: two at most) of the N x N pair terms and runs their sums over j ascending as one chain
// each, T_j (quantile) or p'_k and Tz_k (categorical) read from LDS as broadcasts.  theta_i / the logit of row i stay in
// the owning thread's registers: nothing else reads them.  Values: one wave per row triplet.
// Select: the values kernel's wave per row, then lane 0 draws the row's epsilon-greedy action - what an
// evaluator step and an acting step need from Z in one launch.
//
// The fixed orders (every quantile operation is a separately rounded fp32 operation; the file is built without contraction):
//   S(x, n), the sum of n values used for every sum that is not a chain over j: lane l of one wave chains x[l], x[l + 64], ..
//   ascending from +0; the 64 partials meet in an xor butterfly (offsets 32, 16, .., 1: fp addition commutes, so every lane
//   ends with the same bits).
//   quantile  Q[a] = S(Z[a][:], N) / N;  tau_i = (i + 0.5) / N;  T_j = returns + (live * z_next[a*][j]);
//             u = T_j - theta_i;  h = |u| <= 1 ? (0.5 u) u : |u| - 0.5;  omega = |tau_i - (u < 0 ? 1 : 0)|;
//             sh_i = chain_j (sh + omega h), sg_i = chain_j (sg + omega clamp(u)), both from +0;
//             L_b = S(sh_i / N, N);  dz = (w ((-sg_i) / N)) / B;  loss = S(w_b L_b, B) / B.
//   categorical (held to a float64 restatement within a derived bound, not bit for bit): z_k = v_min + k D;
//             softmax rows: max, e_k = expf(x_k - max), sum S(e, N); value = S(e_k z_k, N) / S(e, N);
//             m_i = chain_k (m + p'_k max(0, 1 - |Tz_k - z_i| (1 / D)));  log p_i = (x_i - max) - logf(S(e, N));
//             L_b = -S(m_i log p_i, N);  M = S(m, N);  dz = (w (expf(log p_i) M - m_i)) / B.
// A clamp or a max that met a NaN keeps it (comparisons, not fminf / fmaxf): non-finite inputs propagate.  No floating-point
// atomics; the only atomic is the integer OR into the model's sticky flag.  Ragged N: a lane or thread whose i is >= N loads
// and stores nothing.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "dist_loss.h"
#include "head_wide.h"
#include "objects.h"
#include "qnet.h"

namespace qlx {

namespace {

constexpr uint32_t kDlMaxStates = 8192, kDlMaxTrain = 4096;
constexpr uint32_t kDlFlagAction = 2u;   // model_dev.hip's kFlagAction: "action out of range (>= 3) in a device call"
constexpr int kPerLane = 6;              // ceil(341 / 64): a wave's share of one row of atoms
constexpr int kRows = 2;                 // ceil(341 / 256): a thread's share of the rows of a loss block
constexpr int kLds = 344;

struct Atoms {
  int N;
  float v_min, v_max, delta, inv_delta;
};

__device__ __forceinline__ float atom(const Atoms& A, int k) { return __fadd_rn(A.v_min, __fmul_rn((float)k, A.delta)); }

__device__ __forceinline__ float butterfly_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = __fadd_rn(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float butterfly_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// S(f(0 .. n - 1)) for n <= 384, by one whole wave
template <class F>
__device__ __forceinline__ float wave_sum(int n, int lane, F f) {
  float acc = 0.0f;
#pragma unroll
  for (int k = 0; k < kPerLane; ++k) {
    const int i = lane + 64 * k;
    if (i < n) acc = __fadd_rn(acc, f(i));
  }
  return butterfly_sum(acc);
}

__device__ __forceinline__ float clampf(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

struct RowStats {
  float mx, sum, value;
};

// softmax statistics of one row of N logits, by one whole wave: the maximum, sum exp(x - max) and the expectation
__device__ __forceinline__ RowStats softmax_row(const float* __restrict__ x, const Atoms& A, int lane) {
  float xv[kPerLane];
  float mx = -__builtin_huge_valf();
#pragma unroll
  for (int k = 0; k < kPerLane; ++k) {
    const int i = lane + 64 * k;
    xv[k] = i < A.N ? x[i] : 0.0f;
    if (i < A.N) mx = fmaxf(mx, xv[k]);
  }
  mx = butterfly_max(mx);
  float s = 0.0f, t = 0.0f;
#pragma unroll
  for (int k = 0; k < kPerLane; ++k) {
    const int i = lane + 64 * k;
    if (i < A.N) {
      const float e = expf(__fsub_rn(xv[k], mx));
      s = __fadd_rn(s, e);
      t = __fadd_rn(t, __fmul_rn(e, atom(A, i)));
    }
  }
  RowStats r;
  r.mx = mx;
  r.sum = butterfly_sum(s);
  r.value = __fdiv_rn(butterfly_sum(t), r.sum);
  return r;
}

__device__ __forceinline__ float quantile_value(const float* __restrict__ x, int N, int lane) {
  return __fdiv_rn(wave_sum(N, lane, [&](int i) { return x[i]; }), (float)N);
}

__device__ __forceinline__ int first_argmax3(float q0, float q1, float q2) {
  int best = 0;
  float top = q0;
  if (q1 > top) { best = 1; top = q1; }
  if (q2 > top) best = 2;
  return best;
}

// ---------------------------------------------------------------------------------------------------------------
// Values: wave w of a block takes row triplet 4 blockIdx + w.
template <int KIND>
__global__ __launch_bounds__(256) void k_dist_values(const float* __restrict__ z, Atoms A, uint32_t n, float* __restrict__ q,
                                                     uint8_t* __restrict__ actions, float* __restrict__ max_q) {
  const int lane = threadIdx.x & 63;
  const uint32_t s = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (s >= n) return;   // (wave-uniform; the kernel has no barrier)
  const float* row = z + (size_t)s * 3 * A.N;
  float qv[3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
    qv[a] = KIND == QLX_DIST_QUANTILE ? quantile_value(row + a * A.N, A.N, lane) : softmax_row(row + a * A.N, A, lane).value;
  if (lane != 0) return;
  const int best = first_argmax3(qv[0], qv[1], qv[2]);
  if (q) {
    q[(size_t)s * 3] = qv[0];
    q[(size_t)s * 3 + 1] = qv[1];
    q[(size_t)s * 3 + 2] = qv[2];
  }
  if (actions) actions[s] = (uint8_t)best;
  if (max_q) max_q[s] = best == 0 ? qv[0] : best == 1 ? qv[1] : qv[2];
}

// ---------------------------------------------------------------------------------------------------------------
// Values, first argmax and the epsilon-greedy draw in one launch: k_dist_values' layout (wave w of a block
// takes forward row 4 blockIdx + w; no LDS, no barrier) and its device functions, so q, the argmax and max-Q are its bits;
// then lane 0 does for the row what evaluator.hip's k_eval_select does.  list: row r is env list[r], valid while
// r < count[1] and kdone[e] < K (the evaluator); null: e = r and every row is valid (the acting call).  A row that is not
// valid reads no Z and leaves nothing behind.  Action counts are integer atomics, one per valid row.
struct SelectArgs {
  const float* z;               // [rows][3 N]
  uint32_t rows;
  const uint32_t* list;         // [rows] or null
  const uint32_t* count;        // with list
  const uint32_t* kdone;        // with list
  uint32_t K;
  double epsilon;
  uint64_t seed;
  uint32_t t, purpose;
  uint8_t* actions;             // [e]
  float* qmax;                  // [e] greedy max-Q, or null
  float* q;                     // [r][3] greedy values, or null
  unsigned long long* counts;   // [3] with list, or null
};

template <int KIND>
__global__ __launch_bounds__(256) void k_dist_select(SelectArgs S, Atoms A) {
  const int lane = threadIdx.x & 63;
  const uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (r >= S.rows) return;   // (wave-uniform, as every exit below)
  uint32_t e = r;
  if (S.list) {
    if (r >= S.count[1]) return;
    e = S.list[r];
    if (S.kdone[e] >= S.K) return;
  }
  const float* row = S.z + (size_t)r * 3 * A.N;
  float qv[3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
    qv[a] = KIND == QLX_DIST_QUANTILE ? quantile_value(row + a * A.N, A.N, lane) : softmax_row(row + a * A.N, A, lane).value;
  if (lane != 0) return;
  const int best = first_argmax3(qv[0], qv[1], qv[2]);
  bool random = false;
  if (S.epsilon > 0.0) {
    RngStreamRegs su(S.seed, e, S.t, S.purpose, 0);   // (no indexed array: no scratch)
    random = S.epsilon > uniform_f64_01(su);
  }
  uint32_t a = (uint32_t)best;
  if (random) {
    RngStreamRegs sa(S.seed, e, S.t, S.purpose, 2);
    a = uniform_u8(sa, kActions);
  }
  S.actions[e] = (uint8_t)a;
  if (S.qmax) S.qmax[e] = best == 0 ? qv[0] : best == 1 ? qv[1] : qv[2];
  if (S.q) {
    S.q[(size_t)r * 3] = qv[0];
    S.q[(size_t)r * 3 + 1] = qv[1];
    S.q[(size_t)r * 3 + 2] = qv[2];
  }
  if (S.counts) atomicAdd(S.counts + a, 1ull);
}

struct LossArgs {
  const float* z;
  qlx_dist_batch b;
  uint32_t B;
  float* dz;
  float* sample_loss;
  uint8_t* a_star_out;
  uint32_t* flag;
};

// the taken action and a* of sample b, checked (>= 3: 0 and the flag); uniform over the block
template <int KIND>
__device__ __forceinline__ void sample_actions(const LossArgs& L, const Atoms& A, uint32_t b, int lane, int& a, int& as,
                                               RowStats (&next)[3]) {
  bool bad = false;
  a = L.b.actions[b];
  if (a >= kActions) { a = 0; bad = true; }
  const float* zn = L.b.z_next + (size_t)b * 3 * A.N;
  if (L.b.a_star) {
    as = L.b.a_star[b];
    if (as >= kActions) { as = 0; bad = true; }
    if (KIND == QLX_DIST_CATEGORICAL) next[0] = softmax_row(zn + as * A.N, A, lane);
  } else if (KIND == QLX_DIST_QUANTILE) {
    as = first_argmax3(quantile_value(zn, A.N, lane), quantile_value(zn + A.N, A.N, lane), quantile_value(zn + 2 * A.N, A.N, lane));
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) next[k] = softmax_row(zn + k * A.N, A, lane);
    as = first_argmax3(next[0].value, next[1].value, next[2].value);
    next[0] = as == 0 ? next[0] : as == 1 ? next[1] : next[2];
  }
  if (threadIdx.x == 0) {
    if (bad) atomicOr(L.flag, kDlFlagAction);
    if (L.a_star_out) L.a_star_out[b] = (uint8_t)as;
  }
}

// the columns of the dz row that belong to the two other actions
__device__ __forceinline__ void zero_other_columns(float* __restrict__ row, int a, int N) {
  for (int c = threadIdx.x; c < 3 * N; c += blockDim.x)
    if (c < a * N || c >= (a + 1) * N) row[c] = 0.0f;
}

// ---------------------------------------------------------------------------------------------------------------
// Quantile Huber loss.  Every wave finds a* for itself (three S over z_next: no barrier), the block stages T in LDS, then the
// row chains run; wave 0 closes L_b.
__global__ __launch_bounds__(256) void k_dist_loss_quantile(LossArgs L, Atoms A) {
  __shared__ float tgt[kLds], rowl[kLds];
  const int tid = threadIdx.x, lane = tid & 63, T = blockDim.x, N = A.N;
  const uint32_t b = blockIdx.x;
  int a, as;
  RowStats unused[3];
  sample_actions<QLX_DIST_QUANTILE>(L, A, b, lane, a, as, unused);
  const float ret = L.b.returns[b];
  const float live = L.b.terminals[b] ? 0.0f : L.b.discounts[b];
  const float w = L.b.weights ? L.b.weights[b] : 1.0f;
  const float* zn = L.b.z_next + ((size_t)b * 3 + as) * N;
  const float* zr = L.z + ((size_t)b * 3 + a) * N;
  float* drow = L.dz + (size_t)b * 3 * N;
  const float Nf = (float)N, Bf = (float)L.B;
  float theta[kRows], wpos[kRows], wneg[kRows];
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    const int i = tid + r * T;
    theta[r] = 0.0f, wpos[r] = 0.0f, wneg[r] = 0.0f;
    if (i < N) {
      tgt[i] = __fadd_rn(ret, __fmul_rn(live, zn[i]));
      theta[r] = zr[i];
      const float tau = __fdiv_rn(__fadd_rn((float)i, 0.5f), Nf);
      wpos[r] = fabsf(tau);
      wneg[r] = fabsf(__fsub_rn(tau, 1.0f));
    }
  }
  zero_other_columns(drow, a, N);
  __syncthreads();
  float sh[kRows] = {0.0f, 0.0f}, sg[kRows] = {0.0f, 0.0f};
  const bool second = tid + T < N;   // (N > 256 only)
  for (int j = 0; j < N; ++j) {
    const float t = tgt[j];
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
      if (r == 1 && !second) break;
      const float u = __fsub_rn(t, theta[r]), au = fabsf(u);
      const float h = au <= 1.0f ? __fmul_rn(__fmul_rn(0.5f, u), u) : __fsub_rn(au, 0.5f);
      const float om = u < 0.0f ? wneg[r] : wpos[r];
      sh[r] = __fadd_rn(sh[r], __fmul_rn(om, h));
      sg[r] = __fadd_rn(sg[r], __fmul_rn(om, clampf(u, -1.0f, 1.0f)));
    }
  }
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    const int i = tid + r * T;
    if (i < N) {
      rowl[i] = __fdiv_rn(sh[r], Nf);
      drow[a * N + i] = __fdiv_rn(__fmul_rn(w, __fdiv_rn(-sg[r], Nf)), Bf);
    }
  }
  __syncthreads();
  if (tid < 64) {
    const float lb = wave_sum(N, lane, [&](int i) { return rowl[i]; });
    if (lane == 0) L.sample_loss[b] = lb;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Projected cross-entropy.  p' and Tz in LDS, the projection by gather (m_i reads every k: no scatter, no atomics), m and
// m log p in LDS for the two closing sums; every wave forms M for its own rows.
__global__ __launch_bounds__(256) void k_dist_loss_categorical(LossArgs L, Atoms A) {
  __shared__ float pp[kLds], tz[kLds], ms[kLds], ml[kLds];
  const int tid = threadIdx.x, lane = tid & 63, T = blockDim.x, N = A.N;
  const uint32_t b = blockIdx.x;
  int a, as;
  RowStats next[3];
  sample_actions<QLX_DIST_CATEGORICAL>(L, A, b, lane, a, as, next);
  const float ret = L.b.returns[b];
  const float live = L.b.terminals[b] ? 0.0f : L.b.discounts[b];
  const float w = L.b.weights ? L.b.weights[b] : 1.0f;
  const float* zn = L.b.z_next + ((size_t)b * 3 + as) * N;
  const float* zr = L.z + ((size_t)b * 3 + a) * N;
  float* drow = L.dz + (size_t)b * 3 * N;
  const RowStats cur = softmax_row(zr, A, lane);
  const float log_sum = logf(cur.sum);
  float zi[kRows], lp[kRows];
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    const int i = tid + r * T;
    zi[r] = 0.0f, lp[r] = 0.0f;
    if (i < N) {
      zi[r] = atom(A, i);
      pp[i] = __fdiv_rn(expf(__fsub_rn(zn[i], next[0].mx)), next[0].sum);
      tz[i] = clampf(__fadd_rn(ret, __fmul_rn(live, zi[r])), A.v_min, A.v_max);
      lp[r] = __fsub_rn(__fsub_rn(zr[i], cur.mx), log_sum);
    }
  }
  zero_other_columns(drow, a, N);
  __syncthreads();
  float m[kRows] = {0.0f, 0.0f};
  const bool second = tid + T < N;
  for (int k = 0; k < N; ++k) {
    const float p = pp[k], t = tz[k];
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
      if (r == 1 && !second) break;
      float hat = __fsub_rn(1.0f, __fmul_rn(fabsf(__fsub_rn(t, zi[r])), A.inv_delta));
      hat = hat < 0.0f ? 0.0f : hat;
      m[r] = __fadd_rn(m[r], __fmul_rn(p, hat));
    }
  }
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    const int i = tid + r * T;
    if (i < N) {
      ms[i] = m[r];
      ml[i] = __fmul_rn(m[r], lp[r]);
    }
  }
  __syncthreads();
  const float M = wave_sum(N, lane, [&](int i) { return ms[i]; });
  const float Bf = (float)L.B;
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    const int i = tid + r * T;
    if (i < N) drow[a * N + i] = __fdiv_rn(__fmul_rn(w, __fsub_rn(__fmul_rn(expf(lp[r]), M), m[r])), Bf);
  }
  if (tid < 64) {
    const float lb = -wave_sum(N, lane, [&](int i) { return ml[i]; });
    if (lane == 0) L.sample_loss[b] = lb;
  }
}

// loss = S(w_b L_b, B) / B: one wave
__global__ __launch_bounds__(64) void k_dist_loss_sum(const float* __restrict__ sample_loss, const float* __restrict__ weights,
                                                      uint32_t B, float* __restrict__ loss) {
  const uint32_t lane = threadIdx.x;
  float acc = 0.0f;
  for (uint32_t b = lane; b < B; b += 64) acc = __fadd_rn(acc, __fmul_rn(weights ? weights[b] : 1.0f, sample_loss[b]));
  acc = butterfly_sum(acc);
  if (lane == 0) loss[0] = __fdiv_rn(acc, (float)B);
}

Atoms atoms_of(const qlx_dist& d) {
  Atoms A;
  A.N = (int)d.atoms;
  const bool cat = d.kind == QLX_DIST_CATEGORICAL;
  A.v_min = cat ? d.v_min : 0.0f;
  A.v_max = cat ? d.v_max : 0.0f;
  A.delta = cat ? (d.v_max - d.v_min) / (float)(d.atoms - 1) : 0.0f;
  A.inv_delta = cat ? 1.0f / A.delta : 0.0f;
  return A;
}

// everything about a descriptor that can be judged without reading a handle
void check_dist(const qlx_dist* d) {
  QLX_CHECK(d, QLX_E_INVALID, "null dist");
  QLX_CHECK(d->kind == QLX_DIST_QUANTILE || d->kind == QLX_DIST_CATEGORICAL, QLX_E_INVALID,
            "dist->kind must be QLX_DIST_QUANTILE or QLX_DIST_CATEGORICAL");
  if (d->kind == QLX_DIST_QUANTILE) {
    QLX_CHECK(d->atoms >= 1 && d->atoms <= kDistMaxAtoms, QLX_E_INVALID, "dist->atoms must be in 1..341 for quantiles");
  } else {
    QLX_CHECK(d->atoms >= 2 && d->atoms <= kDistMaxAtoms, QLX_E_INVALID, "dist->atoms must be in 2..341 for a categorical head");
    QLX_CHECK(std::isfinite(d->v_min) && std::isfinite(d->v_max) && d->v_min < d->v_max, QLX_E_INVALID,
              "dist->v_min and v_max must be finite with v_min < v_max");
    QLX_CHECK(std::isfinite(d->v_max - d->v_min), QLX_E_INVALID, "dist->v_max - v_min must be finite");
  }
}

void check_batch(const qlx_dist_batch* b, uint32_t batch) {
  QLX_CHECK(b, QLX_E_INVALID, "null batch_in");
  QLX_CHECK(b->actions, QLX_E_INVALID, "null batch_in->actions");
  QLX_CHECK(b->returns, QLX_E_INVALID, "null batch_in->returns");
  QLX_CHECK(b->discounts, QLX_E_INVALID, "null batch_in->discounts");
  QLX_CHECK(b->terminals, QLX_E_INVALID, "null batch_in->terminals");
  QLX_CHECK(b->z_next, QLX_E_INVALID, "null batch_in->z_next");
  QLX_CHECK(batch > 0 && batch <= kDlMaxTrain, QLX_E_INVALID, "batch must be in 1..4096");
}

// what the two acting calls share beside the descriptor
void check_select(uint32_t n, double epsilon, const uint8_t* d_actions) {
  QLX_CHECK(n > 0 && n <= kDlMaxStates, QLX_E_INVALID, "n must be in 1..8192");
  QLX_CHECK(std::isfinite(epsilon) && epsilon >= 0.0 && epsilon <= 1.0, QLX_E_INVALID, "epsilon must be finite and in 0..1");
  QLX_CHECK(d_actions, QLX_E_INVALID, "null d_actions");
}

// the checks that read the head
void check_head(const qlx_head* h, const qlx_dist& d, uint32_t n) {
  QLX_CHECK((int64_t)3 * d.atoms == (int64_t)h->width, QLX_E_INVALID, "3 * dist->atoms is not the head's width");
  QLX_CHECK(n <= h->model->dev_reserved, QLX_E_STATE, "n is above the reserved size: qlx_model_reserve first");
}

}  // namespace

void dist_values(const qlx_dist& d, const float* z, uint32_t n, float* q, uint8_t* actions, float* max_q, hipStream_t s) {
  const Atoms A = atoms_of(d);
  if (d.kind == QLX_DIST_QUANTILE)
    hipLaunchKernelGGL(k_dist_values<QLX_DIST_QUANTILE>, dim3((n + 3) / 4), dim3(256), 0, s, z, A, n, q, actions, max_q);
  else
    hipLaunchKernelGGL(k_dist_values<QLX_DIST_CATEGORICAL>, dim3((n + 3) / 4), dim3(256), 0, s, z, A, n, q, actions, max_q);
  QLX_HIP(hipGetLastError());
  debug_sync(s, "k_dist_values");
}

void dist_select(const qlx_dist& d, const float* z, uint32_t rows, const DistSelectRows* active, double epsilon, uint64_t seed,
                 uint32_t t, uint32_t purpose, uint8_t* actions, float* qmax, float* q, hipStream_t s) {
  const Atoms A = atoms_of(d);
  SelectArgs S{};
  S.z = z; S.rows = rows;
  if (active) { S.list = active->list; S.count = active->count; S.kdone = active->kdone; S.K = active->K; S.counts = active->counts; }
  S.epsilon = epsilon; S.seed = seed; S.t = t; S.purpose = purpose;
  S.actions = actions; S.qmax = qmax; S.q = q;
  if (d.kind == QLX_DIST_QUANTILE)
    hipLaunchKernelGGL(k_dist_select<QLX_DIST_QUANTILE>, dim3((rows + 3) / 4), dim3(256), 0, s, S, A);
  else
    hipLaunchKernelGGL(k_dist_select<QLX_DIST_CATEGORICAL>, dim3((rows + 3) / 4), dim3(256), 0, s, S, A);
  QLX_HIP(hipGetLastError());
  debug_sync(s, "k_dist_select");
}

void dist_check(const qlx_dist* d) { check_dist(d); }

void dist_loss(const qlx_dist& d, const float* z, const qlx_dist_batch& b, uint32_t B, float* dz, float* loss, float* sample_loss,
               uint8_t* a_star_out, uint32_t* flag, hipStream_t s) {
  const Atoms A = atoms_of(d);
  LossArgs L;
  L.z = z; L.b = b; L.B = B; L.dz = dz; L.sample_loss = sample_loss; L.a_star_out = a_star_out; L.flag = flag;
  const int threads = 64 * ((std::min(A.N, 256) + 63) / 64);
  if (d.kind == QLX_DIST_QUANTILE)
    hipLaunchKernelGGL(k_dist_loss_quantile, dim3(B), dim3(threads), 0, s, L, A);
  else
    hipLaunchKernelGGL(k_dist_loss_categorical, dim3(B), dim3(threads), 0, s, L, A);
  QLX_HIP(hipGetLastError());
  debug_sync(s, "k_dist_loss");
  if (loss) {
    hipLaunchKernelGGL(k_dist_loss_sum, dim3(1), dim3(64), 0, s, (const float*)sample_loss, b.weights, B, loss);
    QLX_HIP(hipGetLastError());
    debug_sync(s, "k_dist_loss_sum");
  }
}

}  // namespace qlx

using namespace qlx;

extern "C" {

int32_t qlx_head_values_dev(qlx_head* h, const qlx_dist* dist, const float* d_z, uint32_t n, float* d_q, uint8_t* d_actions,
                            float* d_max_q) {
  return guard([&] {
    QLX_CHECK(h, QLX_E_INVALID, "null head");
    check_dist(dist);
    QLX_CHECK(d_z, QLX_E_INVALID, "null d_z");
    QLX_CHECK(n > 0 && n <= kDlMaxStates, QLX_E_INVALID, "n must be in 1..8192");
    QLX_CHECK(d_q || d_actions || d_max_q, QLX_E_INVALID, "d_q, d_actions and d_max_q are all null");
    const qlx_dist d = *dist;
    check_head(h, d, n);
    QLX_HIP(hipSetDevice(h->model->device));
    dist_values(d, d_z, n, d_q, d_actions, d_max_q, h->model->stream);
  });
}

int32_t qlx_head_dist_loss_dev(qlx_head* h, const qlx_dist* dist, const float* d_z, const qlx_dist_batch* batch_in, uint32_t batch,
                               float* d_dz, float* d_loss, float* d_sample_loss, uint8_t* d_a_star_out) {
  return guard([&] {
    QLX_CHECK(h, QLX_E_INVALID, "null head");
    check_dist(dist);
    QLX_CHECK(d_z, QLX_E_INVALID, "null d_z");
    check_batch(batch_in, batch);
    QLX_CHECK(d_dz, QLX_E_INVALID, "null d_dz");
    const qlx_dist d = *dist;
    check_head(h, d, batch);
    qlx_model* m = h->model;
    QLX_HIP(hipSetDevice(m->device));
    dist_loss(d, d_z, *batch_in, batch, d_dz, d_loss, d_sample_loss ? d_sample_loss : h->d_dist.get(), d_a_star_out,
              m->d_dev_flag.get(), m->stream);
  });
}

int32_t qlx_head_dist_train_dev(qlx_head* h, const qlx_dist* dist, const qlx_states_dev* src, const qlx_dist_batch* batch_in,
                                uint32_t batch, float* d_z_work, float* d_dz_work, float* d_loss, float* d_sample_loss) {
  // every check of the four calls first, so that a failure launches nothing
  int32_t rc = guard([&] {
    QLX_CHECK(h, QLX_E_INVALID, "null head");
    check_dist(dist);
    check_source(src);
    check_batch(batch_in, batch);
    QLX_CHECK(d_z_work, QLX_E_INVALID, "null d_z_work");
    QLX_CHECK(d_dz_work, QLX_E_INVALID, "null d_dz_work");
    check_head(h, *dist, batch);
    check_handles(h->model, *src, batch);
  });
  if (rc != QLX_OK) return rc;
  if ((rc = qlx_head_forward_dev(h, src, batch, d_z_work, nullptr)) != QLX_OK) return rc;
  const uint64_t ticket = h->model->fwd_ticket;
  if ((rc = qlx_head_dist_loss_dev(h, dist, d_z_work, batch_in, batch, d_dz_work, d_loss, d_sample_loss, nullptr)) != QLX_OK) return rc;
  if ((rc = qlx_head_backward_dev(h, src, d_dz_work, nullptr, batch, ticket)) != QLX_OK) return rc;
  return qlx_model_step_dev(h->model, 0);
}

int32_t qlx_head_select_dev(qlx_head* h, const qlx_dist* dist, const float* d_z, uint32_t n, double epsilon, uint64_t seed,
                            uint32_t step, uint8_t* d_actions, float* d_max_q, float* d_q) {
  return guard([&] {
    QLX_CHECK(h, QLX_E_INVALID, "null head");
    check_dist(dist);
    QLX_CHECK(d_z, QLX_E_INVALID, "null d_z");
    check_select(n, epsilon, d_actions);
    const qlx_dist d = *dist;
    check_head(h, d, n);
    QLX_HIP(hipSetDevice(h->model->device));
    dist_select(d, d_z, n, nullptr, epsilon, seed, step, P_ACT_DEV, d_actions, d_max_q, d_q, h->model->stream);
  });
}

int32_t qlx_head_act_dev(qlx_head* h, const qlx_dist* dist, const qlx_states_dev* src, uint32_t n, double epsilon, uint64_t seed,
                         uint32_t step, uint8_t* d_actions, float* d_max_q, float* d_q, float* d_z_work) {
  // every check of the two calls first, so that a failure launches nothing
  int32_t rc = guard([&] {
    QLX_CHECK(h, QLX_E_INVALID, "null head");
    check_dist(dist);
    check_source(src);
    check_select(n, epsilon, d_actions);
    QLX_CHECK(d_z_work, QLX_E_INVALID, "null d_z_work");
    check_head(h, *dist, n);
    check_handles(h->model, *src, n);
  });
  if (rc != QLX_OK) return rc;
  if ((rc = qlx_head_forward_dev(h, src, n, d_z_work, nullptr)) != QLX_OK) return rc;
  return qlx_head_select_dev(h, dist, d_z_work, n, epsilon, seed, step, d_actions, d_max_q, d_q);
}

}  // extern "C"
