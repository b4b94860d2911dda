// Proportional prioritized replay on the device (SURVEY §8f #3, config C5 - beyond the reference, whose replay
// is uniform: replay_buffer.rs:85-137 via self_driving_tf_q_learner.rs:276-296).  Oracle: oracle/learner_ref.h
// SumTree / per_sample and Learner::update's priority write.
//
// Layout: one f32 heap of 2L nodes (L = next power of two >= capacity), leaves t[L + slot] = priority^alpha
// of replay slot `slot` (physical FIFO position), node i = t[2i] + t[2i + 1].  Internal nodes are a pure function
// of the leaves, so instead of walking every changed leaf's path the tree is rebuilt bottom-up once per vector
// step, right before it is sampled: ceil(log2 L / 11) launches, each block reducing 2048 nodes of one level
// through 11 levels in LDS (L = 2^20: 8 MB read + 4 MB written, two launches).
//
// Sampling (one block per update, B draws): u_b = (T / B) * (b + r_b) with r_b = gen_range_f32(0, 1) from
// stream (seed, update, rank, P_PER, word b), descending left iff u < left sum or the right subtree is empty;
// IS weight (len * leaf / T)^-beta, normalised by the batch max.  The slot is returned as the logical replay
// index (0 = oldest) the gather kernels take.
//
// Priority write after a vector step's updates: the |TD| errors of all U*B samples, in (update, sample) order;
// a slot drawn more than once keeps the LAST value (as the oracle's sequential writes do): a claim pass keeps the
// highest flat index per slot with atomicMax, the write pass lets only that index store (and clears its claim).
// per_max (the priority new transitions enter with) is the max over every written value: an integer atomicMax on
// the bits of a positive float.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "objects.h"
#include "per.h"

namespace qlx {

constexpr uint32_t kTreeChunk = 2048;

// x^y for the priorities (|td| + eps)^alpha and the IS weights (len p)^-beta, as the build defines it (DESIGN.md §6;
// oracle/learner_ref.cpp det_powf restates it): exp(y ln x) in binary64 from IEEE basic operations only (+ - * / fma,
// rint, frexp / ldexp), rounded once to binary32.  Library powf differs between the device (OCML) and glibc in the last
// bit now and then, and a one-ulp leaf changes the sum tree's partial sums and so, rarely, a draw; with this definition
// the prioritized learner is bit-exact against the oracle.  Accuracy: relative error ~1e-15 in binary64 before the
// final rounding (within one float ulp of the correctly rounded powf; tests/test_oracle_per.py).
__device__ __forceinline__ float per_powf(float xf, float yf) {
#pragma clang fp contract(off)
  if (__builtin_isnan(yf)) return __builtin_nanf("");   // a NaN exponent: NaN on both sides (no rint of NaN below)
  if (!(xf > 0.0f)) return xf == 0.0f ? (yf > 0.0f ? 0.0f : (yf < 0.0f ? __builtin_inff() : 1.0f)) : __builtin_nanf("");
  if (__builtin_isinf(xf)) return yf > 0.0f ? __builtin_inff() : (yf < 0.0f ? 0.0f : 1.0f);
  int e;
  double m = frexp((double)xf, &e);   // [0.5, 1)
  if (m < 0.70710678118654752440) { m = m * 2.0; e -= 1; }
  const double f = (m - 1.0) / (m + 1.0), s = f * f;
  // ln m = 2 f (1 + s / 3 + s^2 / 5 + ...), |f| <= 0.1716: 12 terms
  double p = 1.0 / 23.0;
#pragma unroll
  for (int i = 10; i >= 0; --i) p = fma(p, s, 1.0 / (double)(2 * i + 1));
  const double lnx = fma((double)e, 0.69314718055994530942, (f * p) * 2.0);
  const double z = (double)yf * lnx;
  if (z > 700.0) return __builtin_inff();
  if (z < -745.0) return 0.0f;
  const double kd = rint(z * 1.44269504088896340736);
  double r = fma(-kd, 6.93147180369123816490e-01, z);   // ln 2 = hi + lo (hi: 32 significant bits)
  r = fma(-kd, 1.90821492927058770002e-10, r);
  double q = 1.0 / 1307674368000.0;                      // 1 / 15!
  double fact = 1307674368000.0;
#pragma unroll
  for (int i = 14; i >= 0; --i) {
    fact = fact / (double)(i + 1);                       // i! (exact: integers < 2^53)
    q = fma(q, r, 1.0 / fact);
  }
  return (float)ldexp(q, (int)kd);
}

// block j reduces nodes [W + j S, W + (j + 1) S) of one level up log2(S) levels, storing every parent
__global__ __launch_bounds__(256) void k_tree_build(float* t, uint32_t W, uint32_t S) {
  __shared__ float cur[kTreeChunk];
  const uint32_t tid = threadIdx.x;
  const uint32_t off = blockIdx.x * S;
  for (uint32_t i = tid; i < S; i += 256) cur[i] = t[W + off + i];
  __syncthreads();
  uint32_t n = S, w = W, o = off;
  while (n > 1) {
    n >>= 1; w >>= 1; o >>= 1;
    float v[kTreeChunk / 2 / 256];
#pragma unroll
    for (uint32_t k = 0; k < kTreeChunk / 2 / 256; ++k) {
      const uint32_t i = tid + k * 256;
      if (i < n) v[k] = cur[2 * i] + cur[2 * i + 1];
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kTreeChunk / 2 / 256; ++k) {
      const uint32_t i = tid + k * 256;
      if (i < n) { cur[i] = v[k]; t[w + o + i] = v[k]; }
    }
    __syncthreads();
  }
}

void per_launch_build(hipStream_t s, float* tree, uint32_t L) {
  for (uint32_t W = L; W > 1;) {
    const uint32_t S = std::min(W, kTreeChunk);
    hipLaunchKernelGGL(k_tree_build, dim3(W / S), dim3(256), 0, s, tree, W, S);
    W /= S;
  }
  QLX_HIP(hipGetLastError());
}

__global__ __launch_bounds__(256) void k_per_sample(const float* t, uint32_t L, uint64_t seed, uint32_t first_update,
                                                    uint32_t rank, uint64_t len, float beta, uint32_t B, uint64_t cap,
                                                    uint64_t start, uint64_t* idx_out, float* w_out) {
  __shared__ float red[4];
  const uint32_t u = blockIdx.x, tid = threadIdx.x;
  const float T = t[1];
  const float seg = T / (float)B;
  float wmax = 0.0f;
  for (uint32_t b = tid; b < B; b += 256) {
    RngStream s(seed, first_update + u, rank, P_PER, b);
    const float r = uniform_f32(s, 0.0f, 1.0f);
    float x = seg * ((float)b + r);
    uint32_t i = 1;
    while (i < L) {
      const float left = t[2 * i], right = t[2 * i + 1];
      if (x < left || right == 0.0f) {
        i = 2 * i;
      } else {
        x -= left;
        i = 2 * i + 1;
      }
    }
    const uint64_t slot = i - L;
    const float p = t[i] / T;
    const float w = per_powf((float)len * p, -beta);
    idx_out[(size_t)u * B + b] = (slot + cap - start) % cap;
    w_out[(size_t)u * B + b] = w;
    wmax = fmaxf(wmax, w);
  }
  for (int o = 32; o > 0; o >>= 1) wmax = fmaxf(wmax, __shfl_xor(wmax, o));
  if ((tid & 63) == 0) red[tid >> 6] = wmax;
  __syncthreads();
  wmax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  for (uint32_t b = tid; b < B; b += 256) w_out[(size_t)u * B + b] = w_out[(size_t)u * B + b] / wmax;
}

void per_launch_sample(hipStream_t s, const float* tree, uint32_t L, uint64_t seed, uint32_t first_update, uint32_t n_updates,
                       uint32_t rank, uint64_t len, float beta, uint32_t B, uint64_t cap, uint64_t start, uint64_t* idx_out,
                       float* w_out) {
  QLX_CHECK(len > 0 && len <= cap && cap <= L && start < cap, QLX_E_INVALID, "prioritized sample: bad replay range");
  hipLaunchKernelGGL(k_per_sample, dim3(n_updates), dim3(256), 0, s, tree, L, seed, first_update, rank, len, beta, B, cap, start,
                     idx_out, w_out);
  QLX_HIP(hipGetLastError());
}

// new transitions (FIFO positions first .. first + n - 1) enter at the largest priority so far
__global__ void k_per_push(float* leaves, uint64_t cap, uint64_t first, uint32_t n, const float* per_max) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) leaves[(first + e) % cap] = *per_max;
}

void per_launch_push(hipStream_t s, float* leaves, uint64_t cap, uint64_t first, uint32_t n, const float* per_max) {
  hipLaunchKernelGGL(k_per_push, dim3((n + 255) / 256), dim3(256), 0, s, leaves, cap, first, n, per_max);
  QLX_HIP(hipGetLastError());
}

__global__ void k_per_claim(const uint64_t* idx, uint32_t n, uint64_t cap, uint64_t start, uint32_t* owner) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) atomicMax(&owner[(start + idx[k]) % cap], k + 1);
}

__global__ void k_per_write(const uint64_t* idx, const float* td_abs, uint32_t n, uint64_t cap, uint64_t start, float alpha,
                            float eps, uint32_t* owner, float* leaves, float* per_max) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const uint64_t slot = (start + idx[k]) % cap;
  const float pr = per_powf(td_abs[k] + eps, alpha);
  if (owner[slot] == k + 1) {
    leaves[slot] = pr;
    owner[slot] = 0;
  }
  atomicMax(reinterpret_cast<uint32_t*>(per_max), f32_bits(pr));
}

void per_launch_update(hipStream_t s, const uint64_t* idx, const float* td_abs, uint32_t n, uint64_t cap, uint64_t start,
                       float alpha, float eps, uint32_t* owner, float* leaves, float* per_max) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_per_claim, dim3((n + 255) / 256), dim3(256), 0, s, idx, n, cap, start, owner);
  hipLaunchKernelGGL(k_per_write, dim3((n + 255) / 256), dim3(256), 0, s, idx, td_abs, n, cap, start, alpha, eps, owner, leaves,
                     per_max);
  QLX_HIP(hipGetLastError());
}

// ---------------- one batch per call (the replay's device-tensor calls) ----------------
// k_per_sample is shaped for the learner: one block per update, 64 of them side by side, each lane's draws one after the
// other, 20 dependent loads per draw at L = 2^20.  One batch alone is a pure dependent-latency problem, so k_per_draw
// resolves three tree levels per round trip: below node i the children lie at t[2i .. 2i + 1], the grandchildren at
// t[4i .. 4i + 3], the great-grandchildren at t[8i .. 8i + 7], each group contiguous and aligned to its size (8, 16 and
// 32 bytes), so the three loads issue together and the three decisions are made in registers - with the binary descent's
// own comparisons and subtractions, in its order, so every draw is k_per_sample's bit for bit.  One 1024-thread workgroup
// (the batch maximum stays inside it), D = ceil(B / 1024) <= 4 draws per lane, all of them in flight in every round.

// one level of the descent over the pair (left, right) below the current node: the bit taken, x and the value reached
__device__ __forceinline__ uint32_t per_step(float left, float right, float& x, float& val) {
  if (x < left || right == 0.0f) {
    val = left;
    return 0u;
  }
  x -= left;
  val = right;
  return 1u;
}

constexpr uint32_t kDrawThreads = 1024;

template <int D>
__global__ __launch_bounds__(kDrawThreads) void k_per_draw(const float* __restrict__ t, uint32_t logL, uint64_t seed,
                                                           uint32_t update, uint32_t rank, uint64_t len, float beta, uint32_t B,
                                                           uint64_t cap, uint64_t start, uint64_t* __restrict__ idx_out,
                                                           float* __restrict__ w_out) {
  __shared__ float red[kDrawThreads / 64];
  const uint32_t tid = threadIdx.x;
  const float T = t[1];
  const float seg = T / (float)B;
  float x[D], val[D];
  uint32_t node[D];
  bool act[D];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const uint32_t b = tid + d * kDrawThreads;
    act[d] = b < B;
    node[d] = 1;
    val[d] = T;   // L = 1: the root is the leaf
    x[d] = 0.0f;
    if (act[d]) {
      RngStream s(seed, update, rank, P_PER, b);
      const float r = uniform_f32(s, 0.0f, 1.0f);
      x[d] = seg * ((float)b + r);
    }
  }
  uint32_t lev = 0;
  for (; lev + 3 <= logL; lev += 3) {   // nodes 8i + 7 < 16 * 2^lev <= 2L
    float2 c[D];
    float4 g[D], h0[D], h1[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
      if (act[d]) {
        const size_t i = node[d];
        c[d] = *reinterpret_cast<const float2*>(t + 2 * i);
        g[d] = *reinterpret_cast<const float4*>(t + 4 * i);
        h0[d] = *reinterpret_cast<const float4*>(t + 8 * i);
        h1[d] = *reinterpret_cast<const float4*>(t + 8 * i + 4);
      }
    }
#pragma unroll
    for (int d = 0; d < D; ++d) {
      if (act[d]) {
        const uint32_t b1 = per_step(c[d].x, c[d].y, x[d], val[d]);
        const uint32_t b2 = per_step(b1 ? g[d].z : g[d].x, b1 ? g[d].w : g[d].y, x[d], val[d]);
        const float4 h = b1 ? h1[d] : h0[d];
        const uint32_t b3 = per_step(b2 ? h.z : h.x, b2 ? h.w : h.y, x[d], val[d]);
        node[d] = 8 * node[d] + 4 * b1 + 2 * b2 + b3;
      }
    }
  }
  if (logL - lev == 2) {   // nodes 4i + 3 < 8 * 2^lev = 2L
    float2 c[D];
    float4 g[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
      if (act[d]) {
        const size_t i = node[d];
        c[d] = *reinterpret_cast<const float2*>(t + 2 * i);
        g[d] = *reinterpret_cast<const float4*>(t + 4 * i);
      }
    }
#pragma unroll
    for (int d = 0; d < D; ++d) {
      if (act[d]) {
        const uint32_t b1 = per_step(c[d].x, c[d].y, x[d], val[d]);
        const uint32_t b2 = per_step(b1 ? g[d].z : g[d].x, b1 ? g[d].w : g[d].y, x[d], val[d]);
        node[d] = 4 * node[d] + 2 * b1 + b2;
      }
    }
  } else if (logL - lev == 1) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      if (act[d]) {
        const float2 c = *reinterpret_cast<const float2*>(t + 2 * (size_t)node[d]);
        node[d] = 2 * node[d] + per_step(c.x, c.y, x[d], val[d]);
      }
    }
  }
  const uint32_t L = 1u << logL;
  float w[D];
  float wmax = 0.0f;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    w[d] = 0.0f;
    if (act[d]) {
      const uint64_t slot = node[d] - L;
      idx_out[tid + d * kDrawThreads] = (slot + cap - start) % cap;
      if (w_out) {
        const float p = val[d] / T;   // val = t[node]: the value the last step reached
        w[d] = per_powf((float)len * p, -beta);
        wmax = fmaxf(wmax, w[d]);
      }
    }
  }
  if (!w_out) return;   // uniform over the workgroup
  for (int o = 32; o > 0; o >>= 1) wmax = fmaxf(wmax, __shfl_xor(wmax, o));
  if ((tid & 63) == 0) red[tid >> 6] = wmax;
  __syncthreads();
  wmax = red[0];
#pragma unroll
  for (uint32_t k = 1; k < kDrawThreads / 64; ++k) wmax = fmaxf(wmax, red[k]);
#pragma unroll
  for (int d = 0; d < D; ++d)
    if (act[d]) w_out[tid + d * kDrawThreads] = w[d] / wmax;
}

void per_launch_draw(hipStream_t s, const float* tree, uint32_t L, uint64_t seed, uint32_t update_idx, uint32_t rank, uint64_t len,
                     float beta, uint32_t B, uint64_t cap, uint64_t start, uint64_t* idx_out, float* w_out) {
  QLX_CHECK(len > 0 && len <= cap && cap <= L && start < cap, QLX_E_INVALID, "prioritized draw: bad replay range");
  QLX_CHECK(B > 0 && B <= 4 * kDrawThreads, QLX_E_INVALID, "prioritized draw: batch must be in 1..4096");
  uint32_t logL = 0;
  while ((1u << logL) < L) ++logL;
  const auto k = B <= kDrawThreads ? k_per_draw<1> : B <= 2 * kDrawThreads ? k_per_draw<2> : k_per_draw<4>;
  hipLaunchKernelGGL(k, dim3(1), dim3(kDrawThreads), 0, s, tree, logL, seed, update_idx, rank, len, beta, B, cap, start, idx_out,
                     w_out);
  QLX_HIP(hipGetLastError());
}

// The priority write's claim / write pair with the data the host cannot see guarded.  An entry is valid iff its index is
// < len and its td_abs is finite and >= 0; only valid entries claim, so "last writer wins" holds among them, and only they
// store (through the claim) and raise per_max.  Both kernels evaluate the same predicate.  (A valid entry's priority is
// finite for alpha <= 1: td_abs + eps <= FLT_MAX.)
__device__ __forceinline__ bool per_entry(const uint64_t* idx, const float* td_abs, uint32_t k, uint64_t len, uint64_t* i,
                                          float* td) {
  *i = idx[k];
  *td = td_abs[k];
  return *i < len && *td >= 0.0f && !__builtin_isinf(*td);   // NaN fails the comparison
}

__global__ void k_per_claim_guarded(const uint64_t* idx, const float* td_abs, uint32_t n, uint64_t len, uint64_t cap,
                                    uint64_t start, uint32_t* owner, uint32_t* flag) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  uint64_t i;
  float td;
  if (per_entry(idx, td_abs, k, len, &i, &td))
    atomicMax(&owner[(start + i) % cap], k + 1);
  else
    atomicOr(flag, 1u);
}

__global__ void k_per_write_guarded(const uint64_t* idx, const float* td_abs, uint32_t n, uint64_t len, uint64_t cap,
                                    uint64_t start, float alpha, float eps, uint32_t* owner, float* leaves, float* per_max) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  uint64_t i;
  float td;
  if (!per_entry(idx, td_abs, k, len, &i, &td)) return;
  const uint64_t slot = (start + i) % cap;
  const float pr = per_powf(td + eps, alpha);
  if (owner[slot] == k + 1) {
    leaves[slot] = pr;
    owner[slot] = 0;
  }
  atomicMax(reinterpret_cast<uint32_t*>(per_max), f32_bits(pr));
}

void per_launch_update_guarded(hipStream_t s, const uint64_t* idx, const float* td_abs, uint32_t n, uint64_t len, uint64_t cap,
                               uint64_t start, float alpha, float eps, uint32_t* owner, float* leaves, float* per_max,
                               uint32_t* flag) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_per_claim_guarded, dim3((n + 255) / 256), dim3(256), 0, s, idx, td_abs, n, len, cap, start, owner, flag);
  hipLaunchKernelGGL(k_per_write_guarded, dim3((n + 255) / 256), dim3(256), 0, s, idx, td_abs, n, len, cap, start, alpha, eps, owner,
                     leaves, per_max);
  QLX_HIP(hipGetLastError());
}

uint32_t per_leaves(uint64_t cap) {
  uint32_t L = 1;
  while (L < cap) L <<= 1;
  return L;
}

void PerState::init(uint64_t capacity, size_t max_samples) {
  QLX_CHECK(capacity >= 1 && capacity <= (1ull << 30), QLX_E_INVALID, "prioritized replay: capacity out of range");
  cap = capacity;
  L = per_leaves(capacity);
  d_tree.alloc(2 * (size_t)L);
  QLX_HIP(hipMemset(d_tree, 0, d_tree.bytes()));
  d_owner.alloc(L);
  QLX_HIP(hipMemset(d_owner, 0, d_owner.bytes()));
  d_max.alloc(1);
  const float one = 1.0f;
  QLX_HIP(hipMemcpy(d_max, &one, sizeof(float), hipMemcpyHostToDevice));
  d_w.alloc(max_samples);
  d_td.alloc(max_samples);
}

}  // namespace qlx

// ---------------- standalone sum tree (C ABI, include/qlx.h) ----------------
using namespace qlx;

struct qlx_sumtree {
  int device = 0;
  hipStream_t stream = nullptr;
  PerState st;
  DeviceBuffer<uint64_t> d_idx;
  DeviceBuffer<float> d_w, d_td;
  void need(size_t n) { d_idx.reserve(n); d_w.reserve(n); d_td.reserve(n); }
};

extern "C" {

int32_t qlx_sumtree_create(uint64_t capacity, int32_t device, qlx_sumtree** out) {
  return guard([&] {
    QLX_CHECK(out, QLX_E_INVALID, "null out");
    auto* t = new qlx_sumtree;
    try {
      t->device = current_device_checked(device);
      QLX_HIP(hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking));
      t->st.init(capacity, 0);
    } catch (...) {
      if (t->stream) (void)hipStreamDestroy(t->stream);
      delete t;
      throw;
    }
    *out = t;
  });
}

int32_t qlx_sumtree_destroy(qlx_sumtree* t) {
  return guard([&] {
    if (!t) return;
    (void)hipStreamSynchronize(t->stream);
    (void)hipStreamDestroy(t->stream);
    delete t;
  });
}

int32_t qlx_sumtree_set_leaves(qlx_sumtree* t, const float* leaves) {
  return guard([&] {
    QLX_CHECK(t && leaves, QLX_E_INVALID, "null argument");
    for (uint64_t i = 0; i < t->st.cap; ++i)
      QLX_CHECK(leaves[i] >= 0.0f && std::isfinite(leaves[i]), QLX_E_INVALID, "leaves must be finite and >= 0");
    QLX_HIP(hipMemcpyAsync(t->st.d_tree + t->st.L, leaves, t->st.cap * 4, hipMemcpyHostToDevice, t->stream));
    per_launch_build(t->stream, t->st.d_tree, t->st.L);
    QLX_HIP(hipStreamSynchronize(t->stream));
  });
}

int32_t qlx_sumtree_get(qlx_sumtree* t, float* leaves, float* total, float* per_max) {
  return guard([&] {
    QLX_CHECK(t, QLX_E_INVALID, "null tree");
    per_launch_build(t->stream, t->st.d_tree, t->st.L);
    if (leaves) QLX_HIP(hipMemcpyAsync(leaves, t->st.d_tree + t->st.L, t->st.cap * 4, hipMemcpyDeviceToHost, t->stream));
    if (total) QLX_HIP(hipMemcpyAsync(total, t->st.d_tree + 1, 4, hipMemcpyDeviceToHost, t->stream));
    if (per_max) QLX_HIP(hipMemcpyAsync(per_max, t->st.d_max, 4, hipMemcpyDeviceToHost, t->stream));
    QLX_HIP(hipStreamSynchronize(t->stream));
  });
}

int32_t qlx_sumtree_sample(qlx_sumtree* t, uint64_t seed, uint32_t first_update, uint32_t n_updates, uint32_t rank, uint64_t len,
                           float beta, uint32_t batch, uint64_t* slots, float* weights) {
  return guard([&] {
    QLX_CHECK(t && slots && weights && batch > 0 && n_updates > 0, QLX_E_INVALID, "bad arguments");
    QLX_CHECK(len >= 1 && len <= t->st.cap, QLX_E_INVALID, "len out of range");
    const size_t n = (size_t)n_updates * batch;
    t->need(n);
    float total = 0.0f;
    QLX_HIP(hipMemcpyAsync(&total, t->st.d_tree + 1, 4, hipMemcpyDeviceToHost, t->stream));
    QLX_HIP(hipStreamSynchronize(t->stream));
    QLX_CHECK(total > 0.0f, QLX_E_STATE, "sum tree is empty");
    per_launch_sample(t->stream, t->st.d_tree, t->st.L, seed, first_update, n_updates, rank, len, beta, batch, t->st.cap, 0,
                      t->d_idx, t->d_w);
    QLX_HIP(hipMemcpyAsync(slots, t->d_idx, n * 8, hipMemcpyDeviceToHost, t->stream));
    QLX_HIP(hipMemcpyAsync(weights, t->d_w, n * 4, hipMemcpyDeviceToHost, t->stream));
    QLX_HIP(hipStreamSynchronize(t->stream));
  });
}

int32_t qlx_sumtree_update(qlx_sumtree* t, const uint64_t* slots, const float* td_abs, uint32_t n, float alpha, float eps) {
  return guard([&] {
    QLX_CHECK(t && (n == 0 || (slots && td_abs)), QLX_E_INVALID, "bad arguments");
    for (uint32_t k = 0; k < n; ++k) QLX_CHECK(slots[k] < t->st.cap, QLX_E_INVALID, "slot out of range");
    t->need(n);
    QLX_HIP(hipMemcpyAsync(t->d_idx, slots, (size_t)n * 8, hipMemcpyHostToDevice, t->stream));
    QLX_HIP(hipMemcpyAsync(t->d_td, td_abs, (size_t)n * 4, hipMemcpyHostToDevice, t->stream));
    per_launch_update(t->stream, t->d_idx, t->d_td, n, t->st.cap, 0, alpha, eps, t->st.d_owner, t->st.d_tree + t->st.L,
                      t->st.d_max);
    per_launch_build(t->stream, t->st.d_tree, t->st.L);
    QLX_HIP(hipStreamSynchronize(t->stream));
  });
}

}  // extern "C"
