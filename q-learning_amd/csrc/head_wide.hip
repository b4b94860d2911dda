// The wide output head of the fp32 Q-net (gfx950): Z = a4 Wh + bh for a caller-chosen width 1..1024 beside
// the model's own 512 -> 3 head, with forward, backward and optimizer step, so that a loss written outside the library
// (dueling, C51, QR-DQN, bootstrapped heads) backpropagates through the hand-written trunk.
//
// Three kernels on v_mfma_f32_16x16x4_f32, each output one fmaf chain in a stated order (the MFMA is a k-ordered fmaf
// chain over its four k, lane group 0 first: qnet32_kernels.h).  The orders are those of the existing head, so a width-3
// head with Wh = W4, bh = b4 reproduces k_head32 / k_head32_dq / SideFc2T bit for bit:
//   forward   Z[b][j]   = (((C0 + C1) + C2) + C3) + bh[j],  Cw = chain over k ascending in [128 w, 128 w + 128) of
//                         a4[b][k] Wh[k][j]                                                         (k_head32)
//   data      dz4[b][k] = a4[b][k] > 0 ? chain : 0; the chain starts at k_head32_dq's over n = 0, 1, 2 of W4[k][n] dq[b][n]
//                         (first product rounded) when the caller gives dq, at 0 otherwise, and continues with
//                         fmaf(Wh[k][j], dz[b][j], .) over j ascending                              (k_head32_dq)
//   weights   dWh[k][j] = chain over b ascending of a4[b][k] dz[b][j]; dbh[j] the same with 1 for a4  (SideFc2T)
// A column's chain reads nothing of another column, and a sample's nothing of another sample: a result depends neither on
// the width, nor on the column's position, nor on the batch it is computed in.  Ragged widths and batches are zero (or
// repeated, never stored) operands of the fragment; no load leaves its array.
// The sign of a zero dz4 is not part of the contract: without dq the data chain starts from the accumulator's +0, so a
// first product of -0 comes out as +0 (k_head32_dq would keep -0); with dq the chain starts at the dq chain's value, which
// can be -0, and any later step whose product is a zero - a dz of 0, or the staged zeros past the width - turns it into
// +0.  Every consumer of dz4 is itself a chain from +0, where the two are the same value.
// The fc1 backward and the conv backward run as they are (f32_backward_dense_dz4, model_backward_conv); clip_by_norm and
// Adam use the Q-net's device functions (update32_dev.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "head_wide.h"
#include "objects.h"
#include "qnet.h"
#define QLX_Q32_NO_KERNELS   // the device helpers of qnet32_kernels.h, not its conv1 kernels
#include "update32_dev.h"

namespace qlx {

using namespace q32;

constexpr uint32_t kHwMaxStates = 8192, kHwMaxTrain = 4096;
constexpr char kHeadMagic[8] = {'Q', 'L', 'X', 'H', 'E', 'A', 'D', '1'};

// ---------------------------------------------------------------------------------------------------------------
// Forward.  Block = 16 samples x the column tiles ct = blockIdx.y, + gridDim.y, ..; wave w chains the k quarter w
// (A = Wh^T rows = 16 columns of Z, B = a4 columns = 16 samples).  The 16 a4 rows are staged in LDS once (k_head32's
// stage and pitch: conflict-free fragment reads); a tile's 32 Wh operands per lane come straight from memory, the next
// tile's (and its bh) in flight while this tile's chains run.  The four quarter sums meet in LDS (two buffers, one
// barrier per tile) and thread (sample, column) adds them in order and stores Z with consecutive columns per lane.
constexpr int kHwPitch = 514;
__global__ __launch_bounds__(256) void k_headw_fwd(const float* __restrict__ a4, const float* __restrict__ wh,
                                                   const float* __restrict__ bh, int n, int width, float* __restrict__ z) {
  __shared__ float part[2][4][64][4];
  __shared__ __attribute__((aligned(16))) float xs[16 * kHwPitch];
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s0 = blockIdx.x * 16;
  const int j = lane & 15, g = lane >> 4;
  const int ntiles = (width + 15) / 16;
  {   // stage: 16 rows x 128 float4 of a4 (8 per thread; rows past n read row s0)
    f32x4 xr[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int f = tid + 256 * r, jj = f >> 7, k4 = f & 127;
      xr[r] = ld4(a4 + (size_t)(s0 + jj < n ? s0 + jj : s0) * 512 + 4 * k4);
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int f = tid + 256 * r, jj = f >> 7, k4 = f & 127;
      f32x2* d = reinterpret_cast<f32x2*>(xs + jj * kHwPitch + 4 * k4);
      d[0] = f32x2{xr[r][0], xr[r][1]};
      d[1] = f32x2{xr[r][2], xr[r][3]};
    }
  }
  // Wh[128 w + 4 t + g][16 ct + j] for t = 0 .. 31 (a column past the width reads the last one and multiplies as 0) and
  // the epilogue thread's bh
  auto loadw = [&](int ct, float (&wv)[32], float& bv) {
    const int col = ct * 16 + j, cc = col < width ? col : width - 1;
    const float* p = wh + (size_t)(128 * wave + g) * width + cc;
#pragma unroll
    for (int t = 0; t < 32; ++t) wv[t] = p[(size_t)(4 * t) * width];
    const int ce = ct * 16 + (tid & 15);
    bv = bh[ce < width ? ce : width - 1];
  };
  float wv[32], wn[32], bv, bn = 0.0f;
  int ct = blockIdx.y;
  loadw(ct, wv, bv);
  __syncthreads();
  float xv[32];
  {
    const float* x = xs + j * kHwPitch + 128 * wave + g;   // a4[s0 + j][128 w + 4 t + g]
#pragma unroll
    for (int t = 0; t < 32; ++t) xv[t] = x[4 * t];
  }
  int buf = 0;
  for (; ct < ntiles; ct += gridDim.y) {   // (block-uniform)
    const int nx = ct + gridDim.y;
    if (nx < ntiles) loadw(nx, wn, bn);
    const bool live = ct * 16 + j < width;
    f32x4 acc = zero4();
#pragma unroll
    for (int t = 0; t < 32; ++t) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(live ? wv[t] : 0.0f, xv[t], acc, 0, 0, 0);
    // lane (j, g): columns 16 ct + 4 g + i of sample s0 + j
#pragma unroll
    for (int i = 0; i < 4; ++i) part[buf][wave][lane][i] = acc[i];
    __syncthreads();
    {
      const int smp = tid >> 4, c = tid & 15, L = (c >> 2) * 16 + smp, i = c & 3;
      const int b = s0 + smp, col = ct * 16 + c;
      const float v = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(part[buf][0][L][i], part[buf][1][L][i]), part[buf][2][L][i]),
                                          part[buf][3][L][i]), bv);
      if (b < n && col < width) z[(size_t)b * width + col] = v;
    }
    buf ^= 1;
#pragma unroll
    for (int t = 0; t < 32; ++t) wv[t] = wn[t];
    bv = bn;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Backward data.  Block = 16 samples x 64 k (blockIdx.y), wave w the 16 k from 64 y + 16 w: A = Wh rows k, B = dz^T columns
// b, so lane (b, g) ends with dz4[b][k .. k + 3], k = 64 y + 16 w + 4 g, one 16-byte store.  The reduction runs over j in
// slabs of 128: the block's Wh [64][128] and dz [16][128] slabs are loaded with consecutive lanes on consecutive j (zeros
// past the width or the batch), every load of a slab in flight at once and the next slab's issued before this slab's
// chains run (registers), then staged in LDS at pitch 130 (fragment reads: 16 rows x 2 j of a half wave on 32 banks).
// The accumulator starts at the dq chain (W4 rows and dq from memory, loaded with the first slab).
constexpr int kDzJ = 128, kDzPitch = 130, kDzK = 64;
__global__ __launch_bounds__(256) void k_headw_dz(const float* __restrict__ a4, const float* __restrict__ wh,
                                                  const float* __restrict__ dz, const float* __restrict__ w4,
                                                  const float* __restrict__ dq, int B, int width, float* __restrict__ dz4) {
  __shared__ float whs[kDzK * kDzPitch];
  __shared__ float dzs[16 * kDzPitch];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s0 = blockIdx.x * 16, k0 = blockIdx.y * kDzK;
  const int n = lane & 15, g = lane >> 4;
  const int c = tid & 127, r = tid >> 7;
  float wr[kDzK / 2], dr[8];
  // a slab's loads only (an element past the width or the batch reads a valid address and is zeroed when it is staged: a
  // select here would wait for the load, and with it for the whole slab, before the chains of the slab in LDS could run)
  auto load = [&](int j0) {
    const int jj = j0 + c, jc = jj < width ? jj : 0;
#pragma unroll
    for (int i = 0; i < kDzK / 2; ++i) wr[i] = wh[(size_t)(k0 + r + 2 * i) * width + jc];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int b = s0 + r + 2 * i;
      dr[i] = dz[(size_t)(b < B ? b : s0) * width + jc];
    }
  };
  load(0);
  // this lane's outputs: sample b, k = kb .. kb + 3
  const int b = s0 + n, bc = b < B ? b : s0, kb = k0 + 16 * wave + 4 * g;
  const f32x4 x4 = ld4(a4 + (size_t)bc * 512 + kb);
  f32x4 acc = zero4();
  if (dq) {   // (kernel-uniform)
    const f32x4 w0 = ld4(w4 + 3 * kb), w1 = ld4(w4 + 3 * kb + 4), w2 = ld4(w4 + 3 * kb + 8);
    const float wv[12] = {w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3], w2[0], w2[1], w2[2], w2[3]};   // W4[kb + e][n] at 3 e + n
    const float d0 = dq[(size_t)bc * 3], d1 = dq[(size_t)bc * 3 + 1], d2 = dq[(size_t)bc * 3 + 2];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = fmaf(wv[3 * e + 2], d2, fmaf(wv[3 * e + 1], d1, __fmul_rn(wv[3 * e], d0)));
  }
  for (int j0 = 0; j0 < width; j0 += kDzJ) {
    __syncthreads();   // the previous slab's fragment reads are done
    const bool ok = j0 + c < width;
#pragma unroll
    for (int i = 0; i < kDzK / 2; ++i) whs[(r + 2 * i) * kDzPitch + c] = ok ? wr[i] : 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) dzs[(r + 2 * i) * kDzPitch + c] = ok && s0 + r + 2 * i < B ? dr[i] : 0.0f;
    __syncthreads();
    load(j0 + kDzJ);   // the next slab (past the last one: valid addresses, never staged), in flight under the chains
    // all 32 steps of the slab, whatever the width: j past it are staged zeros, and fmaf(0, 0, acc) is acc in value - in
    // bits too unless acc is -0, which only the dq chain can start it at (the head note: the sign of a zero is free) - so
    // the fixed count changes no chain's value and the LDS reads run ahead of the MFMAs
    const float* ap = whs + (16 * wave + n) * kDzPitch + g;
    const float* bp = dzs + n * kDzPitch + g;
#pragma unroll
    for (int t = 0; t < kDzJ / 4; ++t) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[4 * t], bp[4 * t], acc, 0, 0, 0);
  }
  if (b < B) {
    f32x4 d;
#pragma unroll
    for (int e = 0; e < 4; ++e) d[e] = x4[e] > 0.0f ? acc[e] : 0.0f;
    *reinterpret_cast<f32x4*>(dz4 + (size_t)b * 512 + kb) = d;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Head weight gradient.  Block (t, y): the 16-row tile t of [a4^T ; 1] (t = 32: the ones row, giving dbh) against the four
// column tiles 64 y + 16 w of dz, one per wave; SideFc2T's chain over b (b on the lane groups), run by every wave for its
// tile.  Per pass of 128 samples the a4 columns [128][16] and the dz columns [128][64] go to LDS (dz at pitch 80: the two
// lane groups of a half wave 16 banks apart), the next pass's loads in flight while this pass's chain runs.
constexpr int kWgHB = 128, kWgPitch = 80;
__global__ __launch_bounds__(256) void k_headw_wgrad(const float* __restrict__ a4, const float* __restrict__ dz, int B, int width,
                                                     float* __restrict__ dwh, float* __restrict__ dbh) {
  __shared__ __attribute__((aligned(16))) float as[kWgHB * 16];
  __shared__ float ds[kWgHB * kWgPitch];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t = blockIdx.x, j0 = blockIdx.y * 64;
  const int n = lane & 15, g = lane >> 4;
  const int c = tid & 63, r = tid >> 6;
  f32x4 ar[2];
  float dr[kWgHB / 4];
  // a pass's loads only; rows past the batch and columns past the width read a valid address and are zeroed when staged
  // (k_headw_dz's reason)
  const int tc = t < 32 ? t : 0, cc = j0 + c < width ? j0 + c : 0;
  auto load = [&](int b0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int q = tid + 256 * i, b = b0 + (q >> 2);
      ar[i] = ld4(a4 + (size_t)(b < B ? b : 0) * 512 + tc * 16 + (q & 3) * 4);
    }
#pragma unroll
    for (int i = 0; i < kWgHB / 4; ++i) {
      const int b = b0 + r + 4 * i;
      dr[i] = dz[(size_t)(b < B ? b : 0) * width + cc];
    }
  };
  load(0);
  const bool live = j0 + 16 * wave < width;   // (wave-uniform)
  const bool okc = j0 + c < width;
  f32x4 acc = zero4();
  // (measured and reverted: the loads of two passes in flight, 256 VGPRs - 21.5 -> 28.6 us at width 4, 29.1 -> 56.5 us at
  // width 600, B = 1024)
  for (int b0 = 0; b0 < B; b0 += kWgHB) {
    __syncthreads();   // the previous pass's LDS reads are done
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int q = tid + 256 * i;
      *reinterpret_cast<f32x4*>(as + q * 4) = t < 32 && b0 + (q >> 2) < B ? ar[i] : zero4();
    }
#pragma unroll
    for (int i = 0; i < kWgHB / 4; ++i) ds[(r + 4 * i) * kWgPitch + c] = okc && b0 + r + 4 * i < B ? dr[i] : 0.0f;
    __syncthreads();
    load(b0 + kWgHB);   // the next pass (past the last one: valid addresses, never staged), in flight under the chain
    if (live) {
      // all 32 steps of the pass, whatever the batch: rows past B are staged zeros and leave the chains unchanged, bit
      // for bit (this accumulator starts at +0, and a sum that started at +0 is never -0), and the LDS reads run ahead
      // of the MFMAs
#pragma unroll
      for (int s = 0; s < kWgHB / 4; ++s) {
        const int bl = 4 * s + g;
        const float av = t < 32 ? as[bl * 16 + n] : (n == 0 ? 1.0f : 0.0f);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, ds[bl * kWgPitch + 16 * wave + n], acc, 0, 0, 0);
      }
    }
  }
  const int col = j0 + 16 * wave + n;
  if (!live || col >= width) return;
  if (t < 32) {
#pragma unroll
    for (int i = 0; i < 4; ++i) dwh[(size_t)(t * 16 + 4 * g + i) * width + col] = acc[i];
  } else if (g == 0) {
    dbh[col] = acc[0];
  }
}

// ---------------------------------------------------------------------------------------------------------------
// clip_by_norm + Adam of Wh and bh, two variables with norms of their own.  Segment partials by kNormSeg's scheme
// (norm32_lane, then ((w0 + w1) + w2) + w3), one 256-thread block per segment; then every Adam block finishes both norms
// from the partials (wave 0: lane chain over the partials lane, lane + 64, .., xor butterfly, safe sqrt: k_update32's
// norms_sum) and steps its elements with adam32_elem.
struct HeadUpd {
  float* w;
  float* m;
  float* v;
  const float* g;
  float* part;       // [nseg_w + 1] partials, then the two norms
  int nseg_w;        // Wh's segments; bh has one
  int64_t off[3];    // 0, 512 width, 513 width
  float alpha, beta1, beta2, eps, clipnorm;
};

__global__ __launch_bounds__(256) void k_headw_norms(HeadUpd U) {
  __shared__ float gs[4];
  const int sg = blockIdx.x, tl = threadIdx.x;
  const int v = sg < U.nseg_w ? 0 : 1;
  const float t = norm32_lane(U.g, U.off, 1.0f, v, sg - (v ? U.nseg_w : 0), tl);
  if ((tl & 63) == 0) gs[tl >> 6] = t;
  __syncthreads();
  if (tl == 0) U.part[sg] = __fadd_rn(__fadd_rn(__fadd_rn(gs[0], gs[1]), gs[2]), gs[3]);
}

constexpr int kHeadSegMax = 256;   // Wh at width 1024: 512 * 1024 / 2048
__global__ __launch_bounds__(256) void k_headw_adam(HeadUpd U) {
  __shared__ float nrm[2];
  const int lane = threadIdx.x & 63;
  if (threadIdx.x < 64) {
    float tw = 0.0f;
#pragma unroll
    for (int i = 0; i < kHeadSegMax / 64; ++i) {
      const int idx = lane + 64 * i;
      tw = __fadd_rn(tw, idx < U.nseg_w ? U.part[idx] : 0.0f);
    }
    float tb = __fadd_rn(0.0f, lane == 0 ? U.part[U.nseg_w] : 0.0f);
    for (int o = 32; o > 0; o >>= 1) tw = __fadd_rn(tw, __shfl_xor(tw, o));
    for (int o = 32; o > 0; o >>= 1) tb = __fadd_rn(tb, __shfl_xor(tb, o));
    if (lane == 0) {
      nrm[0] = tw > 0.0f ? sqrtf(tw) : tw;   // safe sqrt via where(l2sum > 0)
      nrm[1] = tb > 0.0f ? sqrtf(tb) : tb;
      if (blockIdx.x == 0) {
        U.part[U.nseg_w + 1] = nrm[0];
        U.part[U.nseg_w + 2] = nrm[1];
      }
    }
  }
  __syncthreads();
  const float dw = clip_denom(nrm[0], U.clipnorm), db = clip_denom(nrm[1], U.clipnorm);
  const int64_t count = U.off[2];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
    float mi = U.m[i], vi = U.v[i];
    U.w[i] = adam32_elem(U.g[i], 1.0f, U.clipnorm, i < U.off[1] ? dw : db, U.alpha, U.beta1, U.beta2, U.eps, mi, vi, U.w[i]);
    U.m[i] = mi;
    U.v[i] = vi;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// host side

static int head_segs_w(int width) { return (kHeadIn * width + kNormSeg - 1) / kNormSeg; }

void head_step(qlx_head* h, hipStream_t s) {
  const qlx_model* m = h->model;
  // Adam's step size of the update about to run (iterations + 1), as the model's (qnet32.hip adam_args)
  const float tf = (float)(h->iterations + 1);
  const float b1p = std::pow(m->beta1, tf), b2p = std::pow(m->beta2, tf);
  HeadUpd U;
  U.w = h->d_w; U.m = h->d_m; U.v = h->d_v; U.g = h->d_grads; U.part = h->d_part;
  U.nseg_w = head_segs_w(h->width);
  U.off[0] = 0; U.off[1] = h->bias_offset(); U.off[2] = h->count();
  U.alpha = m->lr * std::sqrt(1.0f - b2p) / (1.0f - b1p);
  U.beta1 = m->beta1; U.beta2 = m->beta2; U.eps = m->eps; U.clipnorm = m->clipnorm;
  hipLaunchKernelGGL(k_headw_norms, dim3(U.nseg_w + 1), dim3(256), 0, s, U);
  QLX_HIP(hipGetLastError());
  const int blocks = (int)std::min<int64_t>((h->count() + 255) / 256, 1024);
  hipLaunchKernelGGL(k_headw_adam, dim3(blocks), dim3(256), 0, s, U);
  QLX_HIP(hipGetLastError());
  debug_sync(s, "k_headw_adam");
  h->iterations += 1;
}

void head_forward_launch(qlx_head* h, uint32_t n, float* d_z, hipStream_t st) {
  const int rows = ((int)n + 15) / 16, tiles = (h->width + 15) / 16;
  // about a thousand blocks, else every tile its own (at B = 1024 and width 600 measured alike from 512 to 2,048 blocks,
  // 18.3 to 19.0 us, and 25.0 us at 256)
  const int gy = std::min(tiles, std::max(1, (1024 + rows - 1) / rows));
  hipLaunchKernelGGL(k_headw_fwd, dim3(rows, gy), dim3(256), 0, st, f32_a4(h->model), (const float*)h->d_w,
                     (const float*)(h->d_w + h->bias_offset()), (int)n, h->width, d_z);
  QLX_HIP(hipGetLastError());
  debug_sync(st, "k_headw_fwd");
}

static float* head_var(qlx_head* h, int32_t var, int32_t which) {
  float* base = which == 0 ? h->d_w.get() : which == 1 ? h->d_m.get() : h->d_v.get();
  return base + (var == 0 ? 0 : h->bias_offset());
}
static size_t head_var_count(const qlx_head* h, int32_t var) { return var == 0 ? (size_t)kHeadIn * h->width : (size_t)h->width; }

}  // namespace qlx

using namespace qlx;

extern "C" {

int32_t qlx_head_create(qlx_model* m, uint32_t width, uint64_t seed, qlx_head** out) {
  return guard([&] {
    QLX_CHECK(m, QLX_E_INVALID, "null model");
    QLX_CHECK(out, QLX_E_INVALID, "null out");
    QLX_CHECK(width >= 1 && width <= QLX_HEAD_MAX_WIDTH, QLX_E_INVALID, "width must be in 1..1024");
    QLX_CHECK(m->f32, QLX_E_INVALID, "model: a wide head needs an fp32 model (QLX_ARCH_NATURE_DQN)");
    QLX_CHECK(!m->head, QLX_E_STATE, "the model already has a head");
    QLX_HIP(hipSetDevice(m->device));
    auto* h = new qlx_head;
    try {
      h->model = m;
      h->width = (int)width;
      const size_t count = (size_t)h->count();
      h->d_w.alloc(count);
      h->d_m.alloc(count);
      h->d_v.alloc(count);
      h->d_grads.alloc(count);
      h->d_part.alloc((size_t)head_segs_w(h->width) + 3);
      h->d_zero.alloc((size_t)kHwMaxTrain * 3);
      h->d_dist.alloc((size_t)kHwMaxTrain);
      // Wh: GlorotUniform(fan_in 512, fan_out width) from stream (seed, 10, 0, P_INIT), element i = word order; bh = 0
      std::vector<float> w(count, 0.0f);
      const float limit = std::sqrt(6.0f / (float)(kHeadIn + h->width));
      RngStream rs(seed, kHeadInitVar, 0, P_INIT);
      for (size_t i = 0; i < (size_t)kHeadIn * width; ++i) w[i] = uniform_f32(rs, -limit, limit);
      QLX_HIP(hipStreamSynchronize(m->stream));
      QLX_HIP(hipMemcpy(h->d_w, w.data(), count * 4, hipMemcpyHostToDevice));
      QLX_HIP(hipMemset(h->d_m, 0, count * 4));
      QLX_HIP(hipMemset(h->d_v, 0, count * 4));
      QLX_HIP(hipMemset(h->d_grads, 0, count * 4));
      QLX_HIP(hipMemset(h->d_part, 0, h->d_part.bytes()));
      QLX_HIP(hipMemset(h->d_zero, 0, h->d_zero.bytes()));
      QLX_HIP(hipDeviceSynchronize());
    } catch (...) {
      delete h;
      throw;
    }
    m->head = h;
    m->head_grads = false;
    *out = h;
  });
}

int32_t qlx_head_destroy(qlx_head* h) {
  return guard([&] {
    if (!h) return;
    qlx_model* m = h->model;
    (void)hipSetDevice(m->device);
    (void)hipStreamSynchronize(m->stream);
    if (h->event) (void)hipEventDestroy(h->event);
    m->head = nullptr;
    m->head_grads = false;
    delete h;
  });
}

int32_t qlx_head_width(qlx_head* h) { return h ? h->width : -1; }
int64_t qlx_head_iterations(qlx_head* h) { return h ? h->iterations : -1; }

int32_t qlx_head_get_var(qlx_head* h, int32_t var, int32_t which, float* out) {
  return guard([&] {
    QLX_CHECK(h, QLX_E_INVALID, "null head");
    QLX_CHECK(out, QLX_E_INVALID, "null out");
    QLX_CHECK(var == 0 || var == 1, QLX_E_INVALID, "var must be 0 (Wh) or 1 (bh)");
    QLX_CHECK(which >= 0 && which <= 2, QLX_E_INVALID, "which must be 0 (w), 1 (m) or 2 (v)");
    QLX_HIP(hipSetDevice(h->model->device));
    QLX_HIP(hipStreamSynchronize(h->model->stream));
    QLX_HIP(hipMemcpy(out, head_var(h, var, which), head_var_count(h, var) * 4, hipMemcpyDeviceToHost));
  });
}

int32_t qlx_head_set_var(qlx_head* h, int32_t var, int32_t which, const float* in) {
  return guard([&] {
    QLX_CHECK(h, QLX_E_INVALID, "null head");
    QLX_CHECK(in, QLX_E_INVALID, "null in");
    QLX_CHECK(var == 0 || var == 1, QLX_E_INVALID, "var must be 0 (Wh) or 1 (bh)");
    QLX_CHECK(which >= 0 && which <= 2, QLX_E_INVALID, "which must be 0 (w), 1 (m) or 2 (v)");
    QLX_HIP(hipSetDevice(h->model->device));
    QLX_HIP(hipStreamSynchronize(h->model->stream));
    QLX_HIP(hipMemcpy(head_var(h, var, which), in, head_var_count(h, var) * 4, hipMemcpyHostToDevice));
    if (which == 0) h->model->fwd_reusable = false;   // a kept forward belongs to the weights before this write
  });
}

// the head's file: magic, {width, iterations}, then the three buffers whole (Wh then bh in each) - the model's format
// (model.hip qlx_model_write_checkpoint) with the head's width in place of the parameter count
int32_t qlx_head_write_checkpoint(qlx_head* h, const char* path) {
  return guard([&] {
    QLX_CHECK(h, QLX_E_INVALID, "null head");
    QLX_CHECK(path, QLX_E_INVALID, "null path");
    const size_t count = (size_t)h->count();
    QLX_HIP(hipSetDevice(h->model->device));
    QLX_HIP(hipStreamSynchronize(h->model->stream));
    std::vector<float> buf(count * 3);
    QLX_HIP(hipMemcpy(buf.data(), h->d_w, count * 4, hipMemcpyDeviceToHost));
    QLX_HIP(hipMemcpy(buf.data() + count, h->d_m, count * 4, hipMemcpyDeviceToHost));
    QLX_HIP(hipMemcpy(buf.data() + 2 * count, h->d_v, count * 4, hipMemcpyDeviceToHost));
    FILE* f = std::fopen(path, "wb");
    QLX_CHECK(f, QLX_E_IO, std::string("cannot open ") + path);
    const int64_t hdr[2] = {h->width, h->iterations};
    bool ok = std::fwrite(kHeadMagic, 1, 8, f) == 8 && std::fwrite(hdr, 8, 2, f) == 2 &&
              std::fwrite(buf.data(), 4, buf.size(), f) == buf.size();
    ok = (std::fclose(f) == 0) && ok;
    QLX_CHECK(ok, QLX_E_IO, "head checkpoint write failed");
  });
}

// the whole file is in host memory and judged before the first device copy: a refused file changes nothing of the head
int32_t qlx_head_read_checkpoint(qlx_head* h, const char* path) {
  return guard([&] {
    QLX_CHECK(h, QLX_E_INVALID, "null head");
    QLX_CHECK(path, QLX_E_INVALID, "null path");
    FILE* f = std::fopen(path, "rb");
    QLX_CHECK(f, QLX_E_IO, std::string("cannot open ") + path);
    const size_t count = (size_t)h->count();
    char magic[8];
    int64_t hdr[2];
    std::vector<float> buf(count * 3);
    const bool ok = std::fread(magic, 1, 8, f) == 8 && std::memcmp(magic, kHeadMagic, 8) == 0 && std::fread(hdr, 8, 2, f) == 2 &&
                    hdr[0] == h->width && std::fread(buf.data(), 4, buf.size(), f) == buf.size();
    std::fclose(f);
    QLX_CHECK(ok, QLX_E_IO, "not a qlx head checkpoint of this head's width");
    QLX_HIP(hipSetDevice(h->model->device));
    QLX_HIP(hipStreamSynchronize(h->model->stream));
    QLX_HIP(hipMemcpy(h->d_w, buf.data(), count * 4, hipMemcpyHostToDevice));
    QLX_HIP(hipMemcpy(h->d_m, buf.data() + count, count * 4, hipMemcpyHostToDevice));
    QLX_HIP(hipMemcpy(h->d_v, buf.data() + 2 * count, count * 4, hipMemcpyHostToDevice));
    h->iterations = hdr[1];
    h->model->fwd_reusable = false;   // a kept forward belongs to the weights before this read
  });
}

int32_t qlx_head_forward_dev(qlx_head* h, const qlx_states_dev* src, uint32_t n, float* d_z, float* d_q) {
  return guard([&] {
    QLX_CHECK(h, QLX_E_INVALID, "null head");
    check_source(src);
    QLX_CHECK(n > 0 && n <= kHwMaxStates, QLX_E_INVALID, "n must be in 1..8192");
    QLX_CHECK(d_z, QLX_E_INVALID, "null d_z");
    qlx_model* m = h->model;
    const qlx_states_dev s = *src;
    check_handles(m, s, n);
    QLX_HIP(hipSetDevice(m->device));
    hipStream_t st = m->stream;
    model_forward_trunk(m, states_table(m, s, n), (int)n, st);
    head_forward_launch(h, n, d_z, st);
    if (d_q) {
      Fc2Args a = fc2_args(m, (int)n);
      a.q = d_q;
      model_head(m, 0, a, (int)n, st);
    }
  });
}

// (the reuse rule is qlx_model_backward_dev's)
int32_t qlx_head_backward_dev(qlx_head* h, const qlx_states_dev* src, const float* d_dz, const float* d_dq, uint32_t batch,
                              uint64_t ticket) {
  return guard([&] {
    QLX_CHECK(h, QLX_E_INVALID, "null head");
    check_source(src);
    QLX_CHECK(d_dz, QLX_E_INVALID, "null d_dz");
    QLX_CHECK(batch > 0 && batch <= kHwMaxTrain, QLX_E_INVALID, "batch must be in 1..4096");
    qlx_model* m = h->model;
    const qlx_states_dev s = *src;
    check_handles(m, s, batch);
    QLX_HIP(hipSetDevice(m->device));
    hipStream_t st = m->stream;
    const int B = (int)batch;
    const bool reuse = ticket != 0 && ticket == m->fwd_ticket && m->fwd_reusable && m->last_batch == B && m->fwd_table == m->w.table;
    if (!reuse) model_forward_trunk(m, states_table(m, s, batch), B, st);
    float* dz4 = f32_dz4_begin(m, B);
    const float* a4 = f32_a4(m);
    hipLaunchKernelGGL(k_headw_dz, dim3((B + 15) / 16, kHeadIn / kDzK), dim3(256), 0, st, a4, (const float*)h->d_w, d_dz,
                       (const float*)(m->d_params + var_offset(8)), d_dq, B, h->width, dz4);
    QLX_HIP(hipGetLastError());
    debug_sync(st, "k_headw_dz");
    hipLaunchKernelGGL(k_headw_wgrad, dim3(33, (h->width + 63) / 64), dim3(256), 0, st, a4, d_dz, B, h->width, h->d_grads.get(),
                       h->d_grads + h->bias_offset());
    QLX_HIP(hipGetLastError());
    debug_sync(st, "k_headw_wgrad");
    f32_backward_dense_dz4(m, B, d_dq ? d_dq : h->d_zero.get(), st);   // (a zero dq: dW4 and db4 come out zero)
    model_backward_conv(m, m->w.table, B, st, false);
    m->head_grads = true;
  });
}

int32_t qlx_head_grads_dev(qlx_head* h, float** d_grads_out, uint64_t* count_out) {
  return guard([&] {
    QLX_CHECK(h, QLX_E_INVALID, "null head");
    QLX_CHECK(d_grads_out, QLX_E_INVALID, "null d_grads_out");
    QLX_CHECK(count_out, QLX_E_INVALID, "null count_out");
    *d_grads_out = h->d_grads.get();
    *count_out = (uint64_t)h->count();
  });
}

int32_t qlx_head_copy_weights_dev(qlx_head* dst, qlx_head* src) {
  return guard([&] {
    QLX_CHECK(dst, QLX_E_INVALID, "null dst");
    QLX_CHECK(src, QLX_E_INVALID, "null src");
    QLX_CHECK(dst->model->device == src->model->device, QLX_E_INVALID, "dst and src are on different devices");
    QLX_CHECK(dst->width == src->width, QLX_E_INVALID, "dst and src have different widths");
    if (dst == src) return;
    QLX_HIP(hipSetDevice(dst->model->device));
    hipStream_t ds = dst->model->stream, ss = src->model->stream;
    const bool two = ds != ss;
    if (two) {
      if (!dst->event) QLX_HIP(hipEventCreateWithFlags(&dst->event, hipEventDisableTiming));
      QLX_HIP(hipEventRecord(dst->event, ss));
      QLX_HIP(hipStreamWaitEvent(ds, dst->event, 0));
    }
    QLX_HIP(hipMemcpyAsync(dst->d_w, src->d_w, (size_t)dst->count() * sizeof(float), hipMemcpyDeviceToDevice, ds));
    dst->model->fwd_reusable = false;
    if (two) {   // src's later updates write its weights: behind the copy
      QLX_HIP(hipEventRecord(dst->event, ds));
      QLX_HIP(hipStreamWaitEvent(ss, dst->event, 0));
    }
  });
}

}  // extern "C"
