// Device functions of the fp32 update tail shared by the Q-net's update kernels (qnet32.hip) and the wide head's
// (head_wide.hip): the clip_by_norm segment chain and the per-element clip + Adam arithmetic.  One definition, so a
// variable of either is clipped and stepped with the same roundings in the same order.
#pragma once
#include "qnet32_kernels.h"

namespace qlx {

using namespace q32;

// clip_by_norm segment length: segment j of a variable = its elements [j S, (j + 1) S), S = kNormSeg (qnet32.hip)
constexpr int kNormSeg = 2048;

// thread tl (0 .. 255) of segment j of variable v (elements off[v] ..): its fmaf chain over its eight elements, then its
// wave's xor butterfly (every lane ends with the wave sum); segments past the variable's end chain zeros.
// The loads are split from the chain so a caller can put every segment's loads in flight before the first add: variables
// whose length is a multiple of 4 (all but b4) read through a buffer descriptor spanning the variable, elements past its
// end reading as zeros - no per-lane branch around the loads (round 5: the branchy form serialised the five segment
// rounds of a conv update block).
struct NormLd {
  f32x4 x[2];
};
__device__ __forceinline__ NormLd norm32_load(const float* gall, const int64_t* off, int v, int j, int tl, bool live) {
  const int64_t n = off[v + 1] - off[v];
  const int64_t b = (int64_t)j * kNormSeg;
  const float* g = gall + off[v];   // variable offsets are multiples of 4 floats (16-byte loads)
  NormLd L;
  if (n % 4 == 0) {   // wave-uniform
    const __amdgpu_buffer_rsrc_t rs = buf_rsrc(g, live ? (uint32_t)(n * 4) : 0u);
#pragma unroll
    for (int h = 0; h < 2; ++h) L.x[h] = buf_ld4(rs, (uint32_t)((b + 1024 * h + 4 * tl) * 4), 0);
    return L;
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int64_t i = b + 1024 * h + 4 * tl;
#pragma unroll
    for (int k = 0; k < 4; ++k) L.x[h][k] = live && i + k < n ? g[i + k] : 0.0f;   // zeros leave the chain unchanged
  }
  return L;
}
__device__ __forceinline__ float norm32_chain(const NormLd& L, float scale) {
  float t = 0.0f;
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float y = __fmul_rn(L.x[h][k], scale);
      t = fmaf(y, y, t);
    }
  for (int o = 32; o > 0; o >>= 1) t = __fadd_rn(t, __shfl_xor(t, o));
  return t;
}
__device__ __forceinline__ float norm32_lane(const float* gall, const int64_t* off, float scale, int v, int j, int tl) {
  return norm32_chain(norm32_load(gall, off, v, j, tl, true), scale);
}

// tf.clip_by_norm + ResourceApplyAdam per element, explicit roundings in the oracle's order
__device__ __forceinline__ float adam32_elem(float g, float scale, float clipnorm, float denom, float alpha, float beta1,
                                             float beta2, float eps, float& m, float& v, float w) {
  const float gc = __fmul_rn(__fmul_rn(g, scale), clipnorm) / denom;
  m = __fadd_rn(m, __fmul_rn(__fsub_rn(gc, m), 1.0f - beta1));
  v = __fadd_rn(v, __fmul_rn(__fsub_rn(__fmul_rn(gc, gc), v), 1.0f - beta2));
  return __fsub_rn(w, __fmul_rn(m, alpha) / __fadd_rn(sqrtf(v), eps));
}

}  // namespace qlx
