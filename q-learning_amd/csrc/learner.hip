// SelfDrivingQLearner on one MI355X: the env-step -> replay-sample -> Q-net update loop, vectorised over
// n_envs and enqueued on one HIP stream with no host synchronisation per step.
//
// Reference (restated): self_driving_tf_q_learner.rs:94-116 (new: online + stabilized model, same init),
// :141-233 (learn_episode: epsilon-greedy with pure-random warm-up, epsilon decay per step, replay add,
// train every update_after_actions steps once len > B, Bellman target r + gamma * max Q_target(s') or r
// if done, episode bookkeeping + running_reward), :134-139 (solved), :276-296 (distinct ids).
// Vector-step generalisation (N = 1 is the reference loop): DESIGN.md "Learner semantics".
// What does not depend on the environment (acting, episode books, sampling, read-outs) is learner_core.hip; this file is
// the Breakout vector step, the data-parallel update and the C API.  Snapshots: learner_snapshot.hip.
#include <hip/hip_runtime.h>

#include <rccl/rccl.h>

#include <algorithm>
#include <cstdlib>
#include <cmath>
#include <limits>
#include <cstring>
#include <string>
#include <vector>

#include "learner.h"
#include "qnet.h"
#include "replay_dev.h"
#include "stats.h"

// an RCCL call that must succeed; the message is "<function name>: <RCCL's error text>"
#define QLX_NCCL(call)                                                                                                  \
  do {                                                                                                                  \
    const ncclResult_t r__ = (call);                                                                                    \
    QLX_CHECK(r__ == ncclSuccess, QLX_E_COMM, std::string(#call, std::strchr(#call, '(')) + ": " + ncclGetErrorString(r__)); \
  } while (0)

namespace qlx {

ReplayView replay_view(const qlx_replay* rb);

// ---- replay sample gather: frame pointer tables + metadata of one update ------------------------
// (ycache != null: the Bellman target of each sampled slot is read from the per-slot memo instead, see ycache_fill)
__global__ void k_gather(ReplayView r, const uint64_t* idx, uint32_t B, const uint8_t** tab_s, const uint8_t** tab_sn,
                         uint8_t* act, float* rew, uint8_t* done, const float* ycache, float* y) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const uint64_t i = idx[b];
  const uint8_t* f[4];
  replay_frames(r, i, 0, f);
  for (int j = 0; j < 4; ++j) tab_s[b * 4 + j] = f[j];
  const uint64_t t = (r.total - r.len + i) % r.cap;
  act[b] = r.action[t];
  if (ycache) {
    y[b] = ycache[t];
    return;
  }
  replay_frames(r, i, 1, f);
  for (int j = 0; j < 4; ++j) tab_sn[b * 4 + j] = f[j];
  rew[b] = r.reward[t];
  done[b] = r.done[t];
}

// k_gather for n-step returns (n_step > 1): each sample's window walk (replay_dev.h replay_nstep), then
//   vcache != null (the memo holds v = max_a Q_target(s') per slot): y = R + v[last] * g, or R where the window ends
//     in a done - the whole target, no network pass;
//   vcache == null: s' frame pointers of the window's last transition and R, g, terminal per sample, for the batched
//     target pass and k_nstep_combine.
__global__ __launch_bounds__(256) void k_gather_nstep(ReplayView r, const uint64_t* idx, uint32_t B, uint32_t n_step, float gamma,
                                                      const uint8_t** tab_s, const uint8_t** tab_sn, uint8_t* act, float* ret,
                                                      float* disc, uint8_t* term, const float* vcache, float* y) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const uint64_t i = idx[b];
  const uint8_t* f[4];
  replay_frames(r, i, 0, f);
  for (int j = 0; j < 4; ++j) tab_s[b * 4 + j] = f[j];
  act[b] = r.action[(r.total - r.len + i) % r.cap];
  const NStepWindow w = replay_nstep(r, i, n_step, gamma);
  if (vcache) {
    y[b] = w.terminal ? w.R : __fadd_rn(w.R, __fmul_rn(vcache[w.last_p % r.cap], w.g));
    return;
  }
  replay_frames(r, w.last_i, 1, f);
  for (int j = 0; j < 4; ++j) tab_sn[b * 4 + j] = f[j];
  ret[b] = w.R;
  disc[b] = w.g;
  term[b] = w.terminal ? 1 : 0;
}

// y = R + v * g (R where the window ended in a done), in place over the bootstrap values v the target pass left in y
__global__ __launch_bounds__(256) void k_nstep_combine(uint32_t n, const float* ret, const float* disc, const uint8_t* term, float* y) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  const float R = ret[b];
  y[b] = term[b] ? R : __fadd_rn(R, __fmul_rn(y[b], disc[b]));
}

// s' frame pointers, reward and done of the logical replay indices [i0, i0 + n)
__global__ void k_slot_tables(ReplayView r, uint64_t i0, uint32_t n, const uint8_t** tab_sn, float* rew, uint8_t* done) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  const uint8_t* f[4];
  replay_frames(r, i0 + b, 1, f);
  for (int j = 0; j < 4; ++j) tab_sn[b * 4 + j] = f[j];
  const uint64_t t = (r.total - r.len + i0 + b) % r.cap;
  rew[b] = r.reward[t];
  done[b] = r.done[t];
}

__global__ void k_slot_put(ReplayView r, uint64_t i0, uint32_t n, const float* y, float* ycache) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < n) ycache[(r.total - r.len + i0 + b) % r.cap] = y[b];
}

// this rank's contribution to the global solved() test: running reward, has-history flag, episode count (f64: exact sums),
// and the minimum episode reward of its FIFO (+inf when empty, so the min over ranks ignores it)
__global__ void k_book_local(const Book* book, const float* hist, uint32_t hist_cap, double* gsum, float* gmin) {
  if (threadIdx.x != 0) return;
  const Book b = *book;
  float mn = __builtin_huge_valf();
  for (uint32_t i = 0; i < b.hist_len; ++i) mn = fminf(mn, hist[(b.hist_head + i) % hist_cap]);
  gsum[0] = (double)b.running_reward;
  gsum[1] = b.hist_len > 0 ? 1.0 : 0.0;
  gsum[2] = (double)b.episode_count;
  gmin[0] = mn;
}

__global__ void k_obs_table(const uint8_t* obs, uint32_t n, const uint8_t** table) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n * 4) table[i] = obs + (size_t)i * kFramePix;
}

// at least n zero floats in d_zero (n-step: the zero rewards / dones of the bootstrap passes)
static void zero_reserve(qlx_learner* L, uint32_t n) {
  if (n <= L->d_zero.size()) return;
  QLX_HIP(hipStreamSynchronize(L->stream));
  L->d_zero.reserve(n);
  QLX_HIP(hipMemsetAsync(L->d_zero, 0, L->d_zero.bytes(), L->stream));
}

// Head arguments of a target pass over n transitions: y = r + gamma * max_a Q_target(s') (or r if done), a* from q_select
// if given.  n-step returns: the head leaves the bootstrap value instead, y = 0 + v * 1 (s' is then each window's last one).
static Fc2Args target_head_args(qlx_learner* L, uint32_t n, const float* q_select, const float* rewards, const uint8_t* dones,
                                float* y_out) {
  Fc2Args ta = fc2_args(L->target, (int)n);
  ta.q_select = q_select;
  ta.rewards = rewards;
  ta.dones = dones;
  ta.gamma = L->p.gamma;
  ta.y_out = y_out;
  if (L->n_step > 1) {
    ta.rewards = L->d_zero;
    ta.dones = reinterpret_cast<const uint8_t*>(L->d_zero.get());
    ta.gamma = 1.0f;
  }
  return ta;
}

// Target memo.  With the target net frozen, y = r + gamma * max_a Q_target(s') (or r if done) of a transition is a
// fixed function of the transition, and every kernel of the forward computes each sample's chains independently
// of the rest of its batch, so y can be computed once, when the transition enters the replay, and
// read back at every sampling: bit-identical to the per-batch target pass, which at replay ratio 8 evaluates each
// transition's s' eight times on average.  A write of the target weights from outside (model_pack: dist_init's
// broadcast, the model API) invalidates the memo and the next push recomputes every live slot.
// The per-step fill runs chunks of at most ychunk (= min(n_envs, kF32FwdChunk)) transitions; the rebuild of every live slot
// after a target-weight write runs kF32FwdChunk-sized chunks, growing the memo's chunk buffers and the target workspace
// on first use (with n_envs = 1 and a 1M replay, chunks of n_envs would be 1M launches of each kernel).
// n-step returns (n_step > 1): the memo holds v = max_a Q_target(s') per slot instead - the same head at gamma = 1 over zero
// rewards / dones, as qlx_model_batch_max_q runs it - and the gather combines it with the window's R and gamma^m
// (k_gather_nstep).  v is as fixed a function of the slot as y is, so the fill and the rebuild are the same.
static void ycache_reserve(qlx_learner* L, uint32_t chunk) {
  if (L->n_step > 1) zero_reserve(L, chunk);
  // (d_ytmp grows last: after a regrow that failed part-way it is the one that still says so)
  if (chunk > L->d_ytmp.size()) QLX_HIP(hipStreamSynchronize(L->stream));
  L->d_ytab.reserve((size_t)chunk * 4);
  L->d_yrew.reserve(chunk);
  L->d_ydone.reserve(chunk);
  L->d_ytmp.reserve(chunk);
  model_workspace(L->target, (int)chunk);
}

static void ycache_fill(qlx_learner* L, uint64_t i0, uint64_t n, uint32_t chunk) {
  hipStream_t s = L->stream;
  const ReplayView rv = replay_view(L->rb);
  qlx_model* tg = L->target;
  ycache_reserve(L, chunk);
  for (uint64_t c0 = 0; c0 < n; c0 += chunk) {
    const uint32_t m = (uint32_t)std::min<uint64_t>(chunk, n - c0);
    hipLaunchKernelGGL(k_slot_tables, dim3((m + 255) / 256), dim3(256), 0, s, rv, i0 + c0, m, L->d_ytab, L->d_yrew, L->d_ydone);
    QLX_HIP(hipGetLastError());
    model_forward_trunk(tg, L->d_ytab, (int)m, s, false);
    model_head(tg, 2, target_head_args(L, m, nullptr, L->d_yrew, L->d_ydone, L->d_ytmp), (int)m, s);
    hipLaunchKernelGGL(k_slot_put, dim3((m + 255) / 256), dim3(256), 0, s, rv, i0 + c0, m, L->d_ytmp, L->d_ycache);
    QLX_HIP(hipGetLastError());
  }
  debug_sync(s, "ycache_fill");
}

// Targets of all U updates of one vector step in one pass: the target weights are fixed while the step's
// updates run (a target sync happens only between vector steps) and all U batches were sampled up front
// from the same replay state, so y = r + gamma * max_a Q_target(s') (or r if done) for the U*B sampled
// transitions is one batched forward - the same values as U separate passes.
static void learner_targets(qlx_learner* L, uint32_t U) {
  hipStream_t s = L->stream;
  const uint32_t n = U * L->B;
  const ReplayView rv = replay_view(L->rb);
  {
    ProfScope ps(&L->prof, "gather", s);
    if (L->n_step > 1) {
      hipLaunchKernelGGL(k_gather_nstep, dim3((n + 255) / 256), dim3(256), 0, s, rv, L->d_idx, n, L->n_step, L->p.gamma, L->d_tab_s,
                         L->d_tab_sn, L->d_bact, L->d_nret, L->d_ndisc, L->d_nterm, L->ycache ? L->d_ycache : nullptr, L->d_targets);
      QLX_HIP(hipGetLastError());
    } else {
      hipLaunchKernelGGL(k_gather, dim3((n + 255) / 256), dim3(256), 0, s, rv, L->d_idx, n, L->d_tab_s, L->d_tab_sn, L->d_bact,
                         L->d_brew, L->d_bdone, L->ycache ? L->d_ycache : nullptr, L->d_targets);
      QLX_HIP(hipGetLastError());
    }
  }
  debug_sync(s, "gather");
  if (L->ycache) return;
  const float* q_select = nullptr;
  if (L->ddqn) {   // double DQN: a* = argmax Q_online(s') from the online net as it stands before this step's updates
    qlx_model* on = L->online;
    model_forward_trunk(on, L->d_tab_sn, (int)n, s, false);
    Fc2Args oa = fc2_args(on, (int)n);
    model_head(on, 0, oa, (int)n, s);
    q_select = on->w.q;
  }
  // (measured and not kept, round 3: the pass after its first chunk on a second stream beside the update chain - the chain
  // is latency-bound and every CU the pass holds delays it by more than the pass costs on the learner stream)
  qlx_model* tg = L->target;
  model_workspace(tg, (int)n);
  model_forward_trunk(tg, L->d_tab_sn, (int)n, s, false);
  model_head(tg, 2, target_head_args(L, n, q_select, L->d_brew, L->d_bdone, L->d_targets), (int)n, s);
  if (L->n_step > 1) {
    hipLaunchKernelGGL(k_nstep_combine, dim3((n + 255) / 256), dim3(256), 0, s, n, L->d_nret, L->d_ndisc, L->d_nterm, L->d_targets);
    QLX_HIP(hipGetLastError());
  }
}

static void learner_update(qlx_learner* L, uint32_t u_local) {
  hipStream_t s = L->stream;
  const uint32_t B = L->B;
  qlx_model* on = L->online;
  const uint8_t* const* tab_s = L->d_tab_s + (size_t)u_local * B * 4;
  const uint8_t* bact = L->d_bact + (size_t)u_local * B;
  // online: forward, Huber, backward
  model_forward_trunk(on, tab_s, (int)B, s);
  const float* isw = L->per ? L->prio.d_w + (size_t)u_local * B : nullptr;
  float* td = L->per ? L->prio.d_td + (size_t)u_local * B : nullptr;
  float scale = 1.0f;
  if (!L->comm) {   // no all-reduce: the fp32 path may run the norms / Adam inside the backward launches
    model_backward(on, tab_s, (int)B, bact, L->d_targets + (size_t)u_local * B, L->d_losses + u_local, s, isw, td, true);
  } else if (!L->dp_overlap) {   // one all-reduce of the whole gradient on the learner stream
    model_backward(on, tab_s, (int)B, bact, L->d_targets + (size_t)u_local * B, L->d_losses + u_local, s, isw, td);
    ProfScope ps(&L->prof, "allreduce", s);
    QLX_NCCL(ncclAllReduce(on->d_grads, on->d_grads, (size_t)kNumParams, ncclFloat, ncclSum, L->comm, s));
    scale = 1.0f / (float)L->world;
  } else {
    // Data parallel, two gradient buckets: the dense one (W3, b3, W4, b4: 6.42 of 6.74 MB) is all-reduced on the
    // communicator stream as soon as the fc1 backward produced it, overlapping the conv backward; the conv bucket
    // follows on the learner stream once the dense reduction is done (so the two collectives of the communicator
    // never run at the same time and keep one order on every rank).  Adam then sees both.
    scale = 1.0f / (float)L->world;
    model_backward_dense(on, (int)B, bact, L->d_targets + (size_t)u_local * B, L->d_losses + u_local, s, isw, td);
    QLX_HIP(hipEventRecord(L->ev_dense, s));
    QLX_HIP(hipStreamWaitEvent(L->comm_stream, L->ev_dense, 0));
    const int64_t off_dense = kVarOffsetDense;
    {
      ProfScope ps(&L->prof, "allreduce_dense", L->comm_stream);
      QLX_NCCL(ncclAllReduce(on->d_grads + off_dense, on->d_grads + off_dense, (size_t)(kNumParams - off_dense), ncclFloat, ncclSum,
                             L->comm, L->comm_stream));
    }
    // the dense variables' clip-norm partials of the reduced bucket (a model that keeps them apart: the fp32 net) ride in
    // the conv backward's reduction launch, which waits for this all-reduce (round 6: dp_single_rank 0.963 -> 0.967 of the
    // plain path), or (QLX_DP_FOLD=0) follow it on the communicator stream in a launch of their own
    if (!L->dp_fold) model_norms_dense(on, L->comm_stream, scale);
    QLX_HIP(hipEventRecord(L->ev_reduced, L->comm_stream));
    model_backward_conv(on, tab_s, (int)B, s, false, L->dp_fold ? L->ev_reduced : nullptr, scale);
    QLX_HIP(hipStreamWaitEvent(s, L->ev_reduced, 0));
    {
      ProfScope ps(&L->prof, "allreduce_conv", s);
      QLX_NCCL(ncclAllReduce(on->d_grads, on->d_grads, (size_t)off_dense, ncclFloat, ncclSum, L->comm, s));
    }
  }
  model_norms(on, s, scale);
  model_adam(on, s, scale);
  // (after Adam: d_norms is final; before the next update's forward overwrites w.q)
  L->record_metrics(on->w.q, kActions, on->d_norms, kNumVars, on->clipnorm, bact, L->d_targets + (size_t)u_local * B, isw,
                    L->d_losses + u_local, &L->prof);
  L->update_count += 1;
}

// global solved() inputs (data parallel): this rank's episode statistics, then a 3-double sum and a 1-float min all-reduce
// on the learner stream
static void learner_book_allreduce(qlx_learner* L) {
  hipStream_t s = L->stream;
  hipLaunchKernelGGL(k_book_local, dim3(1), dim3(64), 0, s, L->d_book, L->d_hist, (uint32_t)L->p.episode_reward_history_buffer_len,
                     L->d_gsum, L->d_gmin);
  QLX_HIP(hipGetLastError());
  QLX_NCCL(ncclAllReduce(L->d_gsum, L->d_gsum, 3, ncclFloat64, ncclSum, L->comm, s));
  QLX_NCCL(ncclAllReduce(L->d_gmin, L->d_gmin, 1, ncclFloat, ncclMin, L->comm, s));
}

// the goal solved() tests: Environment::episode_reward_goal_mean (breakout_environment.rs:203-206) unless mocked
static float learner_goal(const qlx_learner* L) {
  return std::isnan(L->p.episode_reward_goal) ? (float)(kNumBricks - 1) : L->p.episode_reward_goal;
}

// learning_update_log (self_driving_tf_q_learner.rs:235-273) as of now
static std::string learner_log(qlx_learner* L) {
  static const char* const kNames[kActions] = {"None", "Left", "Right"};   // BreakoutAction Debug
  return L->update_log(learner_goal(L), kNames, kActions, L->rb->d_action, L->rb->len());
}

static void learner_vector_step(qlx_learner* L, bool train = true) {
  hipStream_t s = L->stream;
  const uint32_t N = L->N;
  const uint64_t step_before = L->step_count;
  // ---- act
  const bool any_greedy = step_before + N >= L->p.epsilon_pure_random_steps;
  if (any_greedy) {
    ProfScope ps(&L->prof, "act_forward", s);
    model_forward_trunk(L->online, L->d_obs_table, (int)N, s, false);
    Fc2Args a = fc2_args(L->online, (int)N);
    model_head(L->online, 0, a, (int)N, s);
  }
  L->select_actions(L->online->w.q, kActions, (uint32_t)L->rank * N, &L->prof);
  debug_sync(s, "act + select");
  // ---- env step (physics + frame) and replay push
  {
    ProfScope ps(&L->prof, "env_step", s, 7190.0 * N);   // state r/w + new frame + action/reward/done
    env_launch_step(L->env, L->d_actions, L->d_rewards, L->d_dones);
  }
  debug_sync(s, "env_step");
  {
    ProfScope ps(&L->prof, "replay_push", s, 2.0 * 7056.0 * N + 10.0 * N);   // frame read + write + metadata
    replay_launch_push(L->rb, L->env, s, L->d_actions, L->d_rewards, L->d_dones);
    L->per_push(L->rb->cap, L->rb->total - N, &L->prof);
  }
  debug_sync(s, "replay_push");
  if (L->ycache) {   // y of the N new transitions (all live slots after a write of the target weights)
    ProfScope ps(&L->prof, "target_memo", s);
    if (L->target->version != L->ycache_version) {
      const uint64_t len = L->rb->len();
      ycache_fill(L, 0, len, (uint32_t)std::max<uint64_t>(L->ychunk, std::min<uint64_t>(len, kF32FwdChunk)));
      L->ycache_version = L->target->version;
    } else {
      const uint64_t len = L->rb->len(), fresh = std::min<uint64_t>(N, len);
      ycache_fill(L, len - fresh, fresh, L->ychunk);
    }
  }
  {
    ProfScope ps(&L->prof, "episode_reset", s);
    L->episode_book(L->env->d_ep_steps);
    env_launch_reset(L->env, L->d_reset, 1);
  }
  debug_sync(s, "episode book + reset");
  if (L->comm && L->world > 1) learner_book_allreduce(L);   // global solved(): every vector step
  // ---- training updates
  L->last_updates = 0;
  if (const uint32_t U = train ? L->updates_due(step_before, L->rb->len()) : 0) {
    const uint64_t len = L->rb->len(), cap = L->rb->cap, start = (L->rb->total - len) % cap;
    L->sample(U, len, cap, start, &L->prof);
    debug_sync(s, "sample");
    learner_targets(L, U);
    for (uint32_t u = 0; u < U; ++u) learner_update(L, u);
    L->write_priorities(U, cap, start, &L->prof);
    L->last_updates = U;
  }
  if (L->target_sync_due(step_before)) {
    QLX_HIP(hipMemcpyAsync(L->target->d_params, L->online->d_params, kNumParams * sizeof(float), hipMemcpyDeviceToDevice, s));
    model_pack(L->target);
  }
  L->vec_steps += 1;
  QLX_HIP(hipGetLastError());
}

}  // namespace qlx

using namespace qlx;

extern "C" {

void qlx_params_default(qlx_params* p) {
  std::memset(p, 0, sizeof(*p));
  p->gamma = 0.99f;
  p->lowest_episode_reward_goal_threshold_pct = 0.9f;
  p->episode_reward_goal = std::numeric_limits<float>::quiet_NaN();   // the env's own goal
  p->epsilon_max = 1.0;
  p->epsilon_min = 0.1;
  p->epsilon_greedy_steps = 1000000.0;
  p->max_steps_per_episode = 10000;
  p->epsilon_pure_random_steps = 50000;
  p->history_buffer_len = 1000000;
  p->update_after_actions = 4;
  p->target_sync_steps = 0;
  p->episode_reward_history_buffer_len = 100;
  p->n_envs = 1;
  p->batch_size = 32;
  p->env_seed = 0x51A5EED;
  p->learner_seed = 1;
  p->init_seed = 2;
  p->per_alpha = 0.6f;   // Schaul et al. 2016 proportional variant
  p->per_beta = 0.4f;
  p->per_eps = 1e-6f;
  p->qnet_precision = QLX_PREC_F32;   // the reference's arithmetic
  p->stats_after_steps = 25000;       // Parameter::default (self_driving_tf_q_learner.rs:63)
}

int32_t qlx_learner_create(const qlx_params* p, int32_t device, qlx_learner** out) {
  return guard([&] {
    QLX_CHECK(p && out, QLX_E_INVALID, "null argument");
    LearnerCore::validate(*p);
    QLX_CHECK(p->qnet_precision == QLX_PREC_F32 || p->qnet_precision == QLX_PREC_BF16, QLX_E_INVALID, "unknown qnet_precision");
    QLX_CHECK(p->qnet_precision == QLX_PREC_BF16 || p->batch_size <= (uint32_t)kF32FwdChunk, QLX_E_INVALID,
              "fp32 batch_size above the forward chunk");
    QLX_CHECK(p->n_step <= QLX_NSTEP_MAX, QLX_E_INVALID, "n_step above QLX_NSTEP_MAX");
    // ABI note (round 4): NaN, not 0, selects the env's own goal.  A caller that zero-fills the struct instead of starting
    // from qlx_params_default would mock a goal of 0, which any Breakout episode reaches: say so once.
    if (p->episode_reward_goal == 0.0f)
      std::fprintf(stderr, "qlx_learner_create: episode_reward_goal is 0 - a mocked goal of 0 (NaN selects the env's own goal; "
                           "start from qlx_params_default)\n");
    current_device_checked(device);
    auto* L = new qlx_learner;
    try {   // a failure part-way releases what was built
      L->init(*p, device);
      L->rank = (int)p->rank;
      L->n_step = std::max<uint32_t>(p->n_step, 1);
      int32_t st;
      st = qlx_env_create(QLX_ENV_BREAKOUT, L->N, p->env_seed, device, &L->env);
      QLX_CHECK(st == QLX_OK, st, qlx_last_error());
      st = qlx_replay_create(p->history_buffer_len, L->N, device, &L->rb);
      QLX_CHECK(st == QLX_OK, st, qlx_last_error());
      const int32_t arch = p->qnet_precision == QLX_PREC_BF16 ? QLX_ARCH_NATURE_DQN_BF16 : QLX_ARCH_NATURE_DQN;
      st = qlx_model_create(arch, p->init_seed, device, &L->online);
      QLX_CHECK(st == QLX_OK, st, qlx_last_error());
      st = qlx_model_create(arch, p->init_seed, device, &L->target);   // same initial weights
      QLX_CHECK(st == QLX_OK, st, qlx_last_error());
      // the memo (chunks of n_envs) and the per-batch target pass (U * B samples) must produce the same y bit for bit
      model_set_batch_invariant(L->target);
      // everything runs on the learner's stream
      adopt_stream(L->env, L->stream);
      adopt_stream(L->rb, L->stream);
      adopt_stream(L->online, L->stream);
      adopt_stream(L->target, L->stream);
      L->env->hashing = false;
      // re-seat env ids for data-parallel ranks (ball launch streams are per global env id)
      if (p->rank != 0) {
        L->env->id_offset = p->rank * L->N;
        env_launch_reset(L->env, nullptr, 0);
      }
      const uint32_t N = L->N, B = L->B;
      L->d_obs_table.alloc((size_t)N * 4);
      L->h_book.alloc(1);
      L->h_gsum.alloc(3);
      L->d_sparsity.alloc(8);
      L->h_sparsity.alloc(8);
      const size_t UB = L->max_samples();
      L->d_tab_s.alloc(UB * 4);
      L->d_tab_sn.alloc(UB * 4);
      hipLaunchKernelGGL(k_obs_table, dim3((N * 4 + 255) / 256), dim3(256), 0, L->stream, L->env->d_obs, N, L->d_obs_table);
      QLX_HIP(hipGetLastError());
      model_workspace(L->online, (int)std::max(N, B));
      const char* tc = std::getenv("QLX_TARGET_CACHE");
      L->ycache = p->target_sync_steps == 0 && !L->ddqn && !(tc && tc[0] == '0');
      if (L->ycache) {
        L->ychunk = std::min<uint32_t>(N, (uint32_t)kF32FwdChunk);
        L->d_ycache.alloc(p->history_buffer_len);
        ycache_reserve(L, L->ychunk);
        L->ycache_version = L->target->version;
      } else {
        model_workspace(L->target, (int)(L->max_updates * B));   // batched target pass (learner_targets)
        if (L->n_step > 1) {
          zero_reserve(L, (uint32_t)UB);
          L->d_nret.alloc(UB);
          L->d_ndisc.alloc(UB);
          L->d_nterm.alloc(UB);
        }
      }
      if (L->ddqn) model_workspace(L->online, (int)(L->max_updates * B));   // + the online pass over s'
      QLX_HIP(hipStreamSynchronize(L->stream));
    } catch (...) {
      qlx_learner_destroy(L);
      throw;
    }
    *out = L;
  });
}

int32_t qlx_learner_destroy(qlx_learner* L) {
  return guard([&] {
    if (!L) return;
    (void)hipSetDevice(L->device);
    (void)hipStreamSynchronize(L->stream);
    if (L->comm_stream) (void)hipStreamSynchronize(L->comm_stream);
    if (L->comm) (void)ncclCommDestroy(L->comm);
    if (L->comm_stream) (void)hipStreamDestroy(L->comm_stream);
    for (hipEvent_t e : {L->ev_dense, L->ev_reduced})
      if (e) (void)hipEventDestroy(e);
    qlx_env_destroy(L->env);
    qlx_replay_destroy(L->rb);
    qlx_model_destroy(L->online);
    qlx_model_destroy(L->target);
    (void)hipStreamDestroy(L->stream);
    delete L;
  });
}

static void learner_step_full(qlx_learner* L, bool train);

int32_t qlx_learner_vector_step(qlx_learner* L) {
  return guard([&] {
    QLX_CHECK(L, QLX_E_INVALID, "null learner");
    QLX_HIP(hipSetDevice(L->device));
    learner_step_full(L, true);
  });
}

int32_t qlx_learner_run(qlx_learner* L, uint64_t n) {
  return guard([&] {
    QLX_CHECK(L, QLX_E_INVALID, "null learner");
    QLX_HIP(hipSetDevice(L->device));
    for (uint64_t i = 0; i < n; ++i) learner_step_full(L, true);
  });
}

int32_t qlx_learner_prefill(qlx_learner* L, uint64_t n) {
  return guard([&] {
    QLX_CHECK(L, QLX_E_INVALID, "null learner");
    QLX_HIP(hipSetDevice(L->device));
    for (uint64_t i = 0; i < n; ++i) learner_step_full(L, false);
  });
}

int32_t qlx_learner_end_episodes(qlx_learner* L, const uint8_t* mask) {
  return guard([&] {
    QLX_CHECK(L && mask, QLX_E_INVALID, "null argument");
    QLX_HIP(hipSetDevice(L->device));
    hipStream_t s = L->stream;
    // the episode bookkeeping of one vector step with zero rewards and the mask as the end condition
    QLX_HIP(hipMemcpyAsync(L->d_reset, mask, L->N, hipMemcpyHostToDevice, s));
    QLX_HIP(hipMemsetAsync(L->d_rewards, 0, L->N * sizeof(float), s));
    L->episode_book(L->env->d_ep_steps, L->d_reset, L->d_dones);
    env_launch_reset(L->env, L->d_dones, 1);
    QLX_HIP(hipMemsetAsync(L->d_dones, 0, L->N, s));
    // data parallel: the global solved() inputs include these episodes at once (a collective: every rank calls this,
    // as bench.py's staggered start does)
    if (L->comm && L->world > 1) learner_book_allreduce(L);
    QLX_HIP(hipStreamSynchronize(s));
  });
}

int32_t qlx_learner_learn_till_mastered(qlx_learner* L, uint64_t max_vector_steps, uint64_t* steps_run) {
  return guard([&] {
    QLX_CHECK(L, QLX_E_INVALID, "null learner");
    QLX_HIP(hipSetDevice(L->device));
    uint64_t i = 0;
    qlx_learner_stats st{};
    for (; i < max_vector_steps; ++i) {
      learner_step_full(L, true);
      const int32_t rc = qlx_learner_stats_get(L, &st);
      QLX_CHECK(rc == QLX_OK, rc, qlx_last_error());
      if (st.solved) { ++i; break; }
    }
    if (steps_run) *steps_run = i;
  });
}

uint64_t qlx_learner_stats_events(const qlx_learner* L) { return L ? L->stats_events : 0; }

int32_t qlx_learner_set_log_callback(qlx_learner* L, void (*cb)(const char* text, void* user), void* user) {
  return guard([&] {
    QLX_CHECK(L, QLX_E_INVALID, "null learner");
    L->log_cb = cb;
    L->log_user = user;
  });
}

int32_t qlx_learner_last_log(qlx_learner* L, char* buf, size_t cap, size_t* len) {
  return guard([&] {
    QLX_CHECK(L, QLX_E_INVALID, "null learner");
    copy_text(L->last_log, buf, cap, len);
  });
}

int32_t qlx_learner_sync(qlx_learner* L) {
  return guard([&] {
    QLX_CHECK(L, QLX_E_INVALID, "null learner");
    QLX_HIP(hipStreamSynchronize(L->stream));
    QLX_HIP(hipDeviceSynchronize());
    L->prof.collect();
  });
}

int32_t qlx_learner_stats_get(qlx_learner* L, qlx_learner_stats* out) {
  return guard([&] {
    QLX_CHECK(L && out, QLX_E_INVALID, "null argument");
    const float goal = learner_goal(L);
    L->stats(goal, L->rb->len(), out);
    if (L->comm && L->world > 1) {
      // data parallel: solved over all ranks' episodes (as of the last vector step) = mean of the ranks' running rewards
      // >= goal and the smallest episode reward of any rank's history >= goal * pct, every rank with a history
      double gs[3];
      float gm;
      QLX_HIP(hipMemcpy(gs, L->d_gsum, sizeof(gs), hipMemcpyDeviceToHost));
      QLX_HIP(hipMemcpy(&gm, L->d_gmin, sizeof(gm), hipMemcpyDeviceToHost));
      out->solved = (gs[1] == (double)L->world && gs[0] / (double)L->world >= (double)goal &&
                     gm >= goal * L->p.lowest_episode_reward_goal_threshold_pct) ? 1 : 0;
    }
  });
}

int32_t qlx_learner_last(qlx_learner* L, uint8_t* actions, float* rewards, uint8_t* dones, float* losses,
                         uint64_t* indices, float* targets, uint32_t* n_updates) {
  return guard([&] {
    QLX_CHECK(L, QLX_E_INVALID, "null learner");
    L->last(actions, rewards, dones, losses, indices, targets, n_updates);
  });
}

int32_t qlx_learner_priorities(qlx_learner* L, float* is_weights, float* leaves, float* per_max) {
  return guard([&] {
    QLX_CHECK(L && L->per, QLX_E_STATE, "learner was created without QLX_LEARNER_PER");
    L->priorities(is_weights, leaves, per_max);
  });
}

// Frame sparsity of the last vector step (diagnostic; synchronises): out[0..3] over its sampled training states (NaN when
// it ran no update), out[4..7] over the current acting frames (the observations the NEXT vector step acts on: the table
// after this step's env step and resets), each {conv1 forward zero steps, conv1 weight-gradient zero steps,
// conv2 background rows, conv3 background rows} as fractions (qnet32.hip k_frame_sparsity)
int32_t qlx_learner_frame_sparsity(qlx_learner* L, double* out) {
  return guard([&] {
    QLX_CHECK(L && out, QLX_E_INVALID, "null argument");
    QLX_HIP(hipSetDevice(L->device));
    frame_sparsity(L->d_tab_s, (int)(L->last_updates * L->B), L->d_sparsity, L->h_sparsity, out, L->stream);
    frame_sparsity(L->d_obs_table, (int)L->N, L->d_sparsity + 4, L->h_sparsity + 4, out + 4, L->stream);
  });
}

int32_t qlx_learner_action_counts(qlx_learner* L, uint64_t* counts) {
  return guard([&] {
    QLX_CHECK(L && counts, QLX_E_INVALID, "null argument");
    L->action_counts(L->rb->d_action, L->rb->len(), kActions, counts);
  });
}

int32_t qlx_learner_episode_rewards(qlx_learner* L, float* out, uint64_t cap, uint64_t* n) {
  return guard([&] {
    QLX_CHECK(L, QLX_E_INVALID, "null learner");
    L->episode_rewards(out, cap, n);
  });
}

int32_t qlx_learner_update_log(qlx_learner* L, char* buf, size_t cap, size_t* len) {
  return guard([&] {
    QLX_CHECK(L, QLX_E_INVALID, "null learner");
    copy_text(learner_log(L), buf, cap, len);
  });
}

int32_t qlx_learner_metrics_enable(qlx_learner* L, uint32_t capacity) {
  return guard([&] {
    QLX_CHECK(L, QLX_E_INVALID, "null learner");
    L->metrics_enable(capacity);
  });
}

int32_t qlx_learner_metrics_info(qlx_learner* L, uint32_t* capacity, uint64_t* recorded, uint64_t* unread) {
  return guard([&] {
    QLX_CHECK(L && capacity && recorded && unread, QLX_E_INVALID, "null argument");
    L->metrics_info(capacity, recorded, unread);
  });
}

int32_t qlx_learner_metrics_read(qlx_learner* L, qlx_update_metrics* out, uint64_t cap, uint64_t* n, uint64_t* dropped) {
  return guard([&] {
    QLX_CHECK(L && out && n && dropped, QLX_E_INVALID, "null argument");
    L->metrics_read(out, cap, n, dropped);
  });
}

}  // extern "C"

// One vector step, then the reference's statistics events (self_driving_tf_q_learner.rs:204-212, 226-230):
// write_checkpoint (when checkpoint_file is set) + learning_update_log once per vector step that crossed a multiple of
// stats_after_steps (stats_after_steps > 0), and once more when an episode ended and solved() holds (whatever
// stats_after_steps is).  The log text goes to the callback (the reference's log::info!) and stays readable through
// qlx_learner_last_log.
static void learner_stats_event(qlx_learner* L) {
  if (L->p.checkpoint_file[0] && L->rank == 0) {   // data parallel: the weights are identical, rank 0 writes the file
    char path[257];
    std::memcpy(path, L->p.checkpoint_file, 256);
    path[256] = 0;
    const int32_t rc = qlx_model_write_checkpoint(L->online, path);
    QLX_CHECK(rc == QLX_OK, rc, qlx_last_error());
  }
  if (L->books().book.hist_len == 0) {
    // the reference's log asserts a finished episode (replay_buffer.rs:105-118 avg/min_episode_reward) and would panic;
    // the library logs the counters instead and keeps running
    L->last_log = "episode: 0, steps: " + std::to_string(L->step_count) + " (no finished episode yet)";
  } else {
    L->last_log = learner_log(L);
  }
  L->stats_events += 1;
  if (L->log_cb) L->log_cb(L->last_log.c_str(), L->log_user);
}

static void learner_step_full(qlx_learner* L, bool train) {
  const uint64_t before = L->step_count;
  learner_vector_step(L, train);
  const uint64_t S = L->p.stats_after_steps;
  if (S > 0 && L->step_count / S != before / S) learner_stats_event(L);
  // solved() after an episode ended in this step (:226-230): one pinned copy of the episode counters (the global sums in
  // data parallel, so every rank takes the same decision), and the full test only when an episode ended (on any rank) and
  // the running reward has reached the goal
  const bool dp = L->comm && L->world > 1;
  QLX_HIP(hipMemcpyAsync(L->h_book, L->d_book, sizeof(Book), hipMemcpyDeviceToHost, L->stream));
  if (dp) QLX_HIP(hipMemcpyAsync(L->h_gsum, L->d_gsum, 3 * sizeof(double), hipMemcpyDeviceToHost, L->stream));
  QLX_HIP(hipStreamSynchronize(L->stream));
  const uint64_t episodes = dp ? (uint64_t)L->h_gsum[2] : L->h_book[0].episode_count;
  const bool ended = episodes != L->seen_episodes;
  L->seen_episodes = episodes;
  const float goal = learner_goal(L);
  const bool may_solve = dp ? (L->h_gsum[1] == (double)L->world && L->h_gsum[0] / (double)L->world >= (double)goal)
                            : (L->h_book[0].hist_len > 0 && L->h_book[0].running_reward >= goal);
  if (ended && may_solve) {
    qlx_learner_stats st{};
    const int32_t rc = qlx_learner_stats_get(L, &st);
    QLX_CHECK(rc == QLX_OK, rc, qlx_last_error());
    if (st.solved) learner_stats_event(L);
  }
}

extern "C" {

qlx_env* qlx_learner_env(qlx_learner* L) { return L ? L->env : nullptr; }

// Policy evaluation of the online model (evaluator.hip) between vector steps: a temporary evaluator with an env batch of
// its own runs on the learner's stream (the model's), so it is ordered after the steps enqueued so far; nothing of the
// learner but the online model's workspace (regrown when cfg->n_envs is above its batch) is touched.
int32_t qlx_learner_evaluate(qlx_learner* L, const qlx_eval_config* cfg, qlx_eval_summary* out) {
  return guard([&] {
    QLX_CHECK(L && cfg && out, QLX_E_INVALID, "null argument");
    qlx_evaluator* ev = nullptr;
    int32_t st = qlx_evaluator_create(cfg, L->device, &ev);
    QLX_CHECK(st == QLX_OK, st, qlx_last_error());
    st = qlx_evaluator_run(ev, L->online, out);
    const std::string msg = st == QLX_OK ? "" : qlx_last_error();
    qlx_evaluator_destroy(ev);
    QLX_CHECK(st == QLX_OK, st, msg);
  });
}
qlx_replay* qlx_learner_replay(qlx_learner* L) { return L ? L->rb : nullptr; }
qlx_model* qlx_learner_model(qlx_learner* L, int32_t which) { return L ? (which == 0 ? L->online : L->target) : nullptr; }

int32_t qlx_dist_unique_id(uint8_t out[128]) {
  return guard([&] {
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    ncclUniqueId id;
    QLX_NCCL(ncclGetUniqueId(&id));
    std::memcpy(out, &id, 128);
  });
}

int32_t qlx_learner_dist_init(qlx_learner* L, int32_t world, int32_t rank, const uint8_t uid[128]) {
  return guard([&] {
    QLX_CHECK(L && uid && world >= 1 && rank >= 0 && rank < world, QLX_E_INVALID, "bad argument");
    QLX_CHECK(rank == L->rank, QLX_E_INVALID, "rank differs from qlx_params.rank");
    QLX_CHECK(!L->comm, QLX_E_STATE, "communicator already initialised");
    // world == 1 builds a single-rank communicator: the data-parallel update path (bucketed all-reduce on its
    // own stream) with identity reductions, for tests on one GPU
    QLX_HIP(hipSetDevice(L->device));
    ncclUniqueId id;
    std::memcpy(&id, uid, 128);
    QLX_NCCL(ncclCommInitRank(&L->comm, world, id, rank));
    // (measured and not kept, round 6: the communicator stream at the device's highest priority - dp_single_rank 0.96 ->
    // 0.41 of the plain path)
    QLX_HIP(hipStreamCreateWithFlags(&L->comm_stream, hipStreamNonBlocking));
    const char* ov = std::getenv("QLX_DP_OVERLAP");
    L->dp_overlap = !(ov && ov[0] == '0');
    const char* fo = std::getenv("QLX_DP_FOLD");
    L->dp_fold = !(fo && fo[0] == '0');
    for (hipEvent_t* e : {&L->ev_dense, &L->ev_reduced}) QLX_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
    L->world = world;
    L->rank = rank;
    L->d_gsum.alloc(3);
    L->d_gmin.alloc(1);
    // rank 0's online weights, Adam slots and step count on every rank (one broadcast of the initial
    // weights), and the target net = the online net as in SelfDrivingQLearner::new (self_driving_tf_q_learner.rs:94-116)
    qlx_model* on = L->online;
    QLX_HIP(hipStreamSynchronize(L->stream));
    DeviceBuffer<int64_t> d_iter(1);
    QLX_HIP(hipMemcpy(d_iter, &on->iterations, sizeof(int64_t), hipMemcpyHostToDevice));
    for (float* buf : {on->d_params.get(), on->d_m.get(), on->d_v.get()})
      QLX_NCCL(ncclBroadcast(buf, buf, (size_t)kNumParams, ncclFloat, 0, L->comm, L->stream));
    QLX_NCCL(ncclBroadcast(d_iter, d_iter, 1, ncclInt64, 0, L->comm, L->stream));
    QLX_HIP(hipMemcpyAsync(L->target->d_params, on->d_params, kNumParams * sizeof(float), hipMemcpyDeviceToDevice, L->stream));
    model_pack(on);
    model_pack(L->target);
    QLX_HIP(hipStreamSynchronize(L->stream));
    QLX_HIP(hipMemcpy(&on->iterations, d_iter, sizeof(int64_t), hipMemcpyDeviceToHost));
    // the global episode statistics as of now, so a stats query before the first vector step reads defined values
    if (world > 1) {
      learner_book_allreduce(L);
      QLX_HIP(hipMemcpyAsync(L->h_gsum, L->d_gsum, 3 * sizeof(double), hipMemcpyDeviceToHost, L->stream));
      QLX_HIP(hipStreamSynchronize(L->stream));
      L->seen_episodes = (uint64_t)L->h_gsum[2];   // the solved() check now follows the global episode count
    }
  });
}

int32_t qlx_learner_comm_size(qlx_learner* L, int32_t* world) {
  return guard([&] {
    QLX_CHECK(L && world, QLX_E_INVALID, "null argument");
    *world = 1;
    if (!L->comm) return;
    int n = 0;
    QLX_NCCL(ncclCommCount(L->comm, &n));
    *world = n;
  });
}

int32_t qlx_learner_profile(qlx_learner* L, int32_t enable) {
  return guard([&] {
    QLX_CHECK(L, QLX_E_INVALID, "null learner");
    QLX_HIP(hipStreamSynchronize(L->stream));
    L->prof.reset();
    L->prof.enabled = enable != 0;
    L->online->prof = enable ? &L->prof : nullptr;
    L->target->prof = enable ? &L->prof : nullptr;
  });
}

int32_t qlx_learner_profile_filter(qlx_learner* L, const char* name) { return qlx_learner_profile_sample(L, name, 1); }

int32_t qlx_learner_profile_sample(qlx_learner* L, const char* name, uint32_t stride) {
  return guard([&] {
    QLX_CHECK(L && stride >= 1, QLX_E_INVALID, "bad argument");
    QLX_HIP(hipStreamSynchronize(L->stream));
    L->prof.collect();
    L->prof.filter = name ? name : "";
    L->prof.stride = stride;
    L->prof.seen = 0;
  });
}

int32_t qlx_learner_profile_get(qlx_learner* L, const char* name, double* total_us, double* total_work,
                                uint64_t* launches) {
  return guard([&] {
    QLX_CHECK(L && name && total_us && total_work && launches, QLX_E_INVALID, "null argument");
    QLX_HIP(hipStreamSynchronize(L->stream));
    L->prof.collect();
    auto it = L->prof.acc.find(name);
    if (it == L->prof.acc.end()) { *total_us = 0.0; *total_work = 0.0; *launches = 0; return; }
    *total_us = it->second.us;
    *total_work = it->second.work;
    *launches = it->second.launches;
  });
}

int32_t qlx_learner_profile_names(qlx_learner* L, char* buf, size_t cap) {
  return guard([&] {
    QLX_CHECK(L && buf && cap > 0, QLX_E_INVALID, "null argument");
    QLX_HIP(hipStreamSynchronize(L->stream));
    L->prof.collect();
    std::string s;
    for (auto& kv : L->prof.acc) { if (!s.empty()) s += ","; s += kv.first; }
    QLX_CHECK(s.size() < cap, QLX_E_INVALID, "buffer too small");
    std::memcpy(buf, s.c_str(), s.size() + 1);
  });
}

}  // extern "C"
