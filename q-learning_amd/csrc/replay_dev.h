// Device-side view of the HBM replay ring (shared by replay.hip and learner.hip).
//
// Layout (frame dedup; ReplayBuffer semantics of replay_buffer.rs:52-138 are preserved):
//   transitions are pushed n_envs at a time, env order, so push position p = vector_step * n + env.
//   frames[F][7056]   F = capacity + 4 * n_envs   the frame each transition produced (s2d layout)
//   action/reward/done/epstep [capacity]          epstep k = 1-based step of the env's episode
// Transition p's states are rebuilt from the frames of the same env at positions p - d * n:
//   s'  slot j : d = (k - 1 - j) mod 4, valid iff k - d >= 1
//   s   slot j : d = 1 + ((k - 2 - j) mod 4), valid iff k - d >= 1          (invalid -> zero frame)
// which is exactly the FrameRingBuffer content (ring slot = (episode step - 1) mod 4, zeros after reset).
#pragma once
#include <cstdint>

#include "qlx_internal.h"

namespace qlx {

struct ReplayView {
  const uint8_t* frames;
  const uint8_t* action;
  const float* reward;
  const uint8_t* done;
  const uint32_t* epstep;
  uint64_t cap, F, total, len;
  uint32_t n;
};

// frame pointers of transition at logical index i (0 = oldest); which: 0 = s, 1 = s'
__device__ __forceinline__ void replay_frames(const ReplayView& r, uint64_t i, int which, const uint8_t* out[4]) {
  const uint64_t p = r.total - r.len + i;
  const int k = (int)r.epstep[p % r.cap];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int d = which ? ((k - 1 - j) & 3) : 1 + ((k - 2 - j) & 3);
    out[j] = (k - d >= 1) ? r.frames + ((p - (uint64_t)d * r.n) % r.F) * kFramePix : nullptr;
  }
}

// n-step window of the transition at logical index i (DESIGN.md §6 "n-step returns"): the same env's next transition
// sits n_envs push positions on, and a window ends after n transitions, at a done, at the newest pushed transition,
// or where the next slot's epstep is not this one's + 1 (an episode that ended without a done: the
// max_steps_per_episode cut, qlx_learner_end_episodes).  R = sum_{j<m} gamma^j r_j and g = gamma^m in fp32 with
// one rounding per multiply and per add (no FMA); m = 1 gives R = r, g = gamma, last = i.
struct NStepWindow {
  float R, g;
  uint32_t m;        // transitions in the window, 1 .. n
  uint64_t last_p;   // push position of the window's last transition
  uint64_t last_i;   // its logical index
  bool terminal;     // done[last]
};

__device__ __forceinline__ NStepWindow replay_nstep(const ReplayView& r, uint64_t i, uint32_t n, float gamma) {
  // HIP's __fmul_rn / __fadd_rn are plain * and + that the default contraction mode may still fuse (replay.hip is not
  // built with -ffp-contract=off), so the two roundings per term are the bare operators under this pragma
#pragma clang fp contract(off)
  const uint64_t base = r.total - r.len;
  uint64_t q = base + i;
  NStepWindow w;
  w.g = 1.0f;
  w.R = 0.0f;
  w.m = 0;
  for (;;) {
    const uint64_t t = q % r.cap;
    const float rw = r.reward[t];
    w.R = w.m == 0 ? rw : w.R + w.g * rw;
    w.g = w.g * gamma;
    w.m += 1;
    w.terminal = r.done[t] != 0;
    if (w.m == n || w.terminal || q + r.n >= r.total) break;
    if (r.epstep[(q + r.n) % r.cap] != r.epstep[t] + 1) break;
    q += r.n;
  }
  w.last_p = q;
  w.last_i = q - base;
  return w;
}

}  // namespace qlx
