// The environment-independent half of a learner (learner_core.h), shared by the Breakout and the BallGame learner.
//
// Reference (restated): self_driving_tf_q_learner.rs:141-233 (learn_episode: epsilon-greedy with pure-random warm-up,
// epsilon decay per step, train every update_after_actions steps once len > B, episode bookkeeping + running_reward),
// :134-139 (solved), :235-273 (learning_update_log).  Vector-step generalisation: DESIGN.md "Learner semantics".
#include "learner_core.h"

#include <algorithm>
#include <cmath>

#include "metrics.h"
#include "objects.h"
#include "profiler.h"
#include "stats.h"

namespace qlx {

// ---- acting: epsilon-greedy (self_driving_tf_q_learner.rs:153-167) --------------------------
// step_count of env e in this vector step = step_before + e + 1; epsilon used = eps_table[step_count - 1]
// (value after step_count - 1 decrements). Draws: f64 from words 0-1, the random action from word 2 on.
__global__ void k_select_actions(uint32_t n, uint32_t n_actions, uint64_t step_before, uint64_t pure_random,
                                 const double* eps_table, uint64_t eps_len, double eps_min, uint64_t seed, uint32_t id_offset,
                                 uint32_t vec_step, const float* q, uint8_t* actions) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const uint64_t sc = step_before + e + 1;
  bool random = sc < pure_random;
  if (!random) {
    RngStream su(seed, id_offset + e, vec_step, P_ACT, 0);
    const double eps = (sc - 1) < eps_len ? eps_table[sc - 1] : eps_min;
    random = eps > uniform_f64_01(su);
  }
  uint8_t a;
  if (random) {
    RngStream sa(seed, id_offset + e, vec_step, P_ACT, 2);
    a = (uint8_t)uniform_u8(sa, n_actions);
  } else {   // tf.argmax over Q(s): first maximal index
    int best = 0;
    float bv = q[e * n_actions];
    for (uint32_t j = 1; j < n_actions; ++j)
      if (q[e * n_actions + j] > bv) { best = (int)j; bv = q[e * n_actions + j]; }
    a = (uint8_t)best;
  }
  actions[e] = a;
}

// ---- episode bookkeeping (learn_episode :172-174, :214-224) -----------------------------------

// Envs in order: ep_reward += r; an env whose episode ended (done, or max_steps_per_episode steps) pushes its
// reward into the FIFO of episode rewards, counts the episode and is marked for reset.  The per-env part runs
// one thread per env (1024 per round); wave 0 then walks the round's endings in env order (ballot per 64 envs)
// and keeps the Book.  running_reward is refreshed (sequential f32 sum, oldest first) by every ending with
// episode_count >= hist cap; only the last such refresh of the step survives and it sums the final FIFO, so it
// runs once: the FIFO is loaded 64 entries per lane-parallel load and summed in order with uniform lane reads.
__global__ __launch_bounds__(1024) void k_episode_book(uint32_t n, const float* rewards, const uint8_t* dones,
                                                       const uint32_t* ep_steps, uint64_t max_steps, float* ep_reward,
                                                       float* hist, uint32_t hist_cap, Book* book, uint8_t* reset_mask) {
  __shared__ float s_er[1024];
  __shared__ uint8_t s_end[1024];
  const int tid = threadIdx.x, lane = tid & 63;
  Book b = *book;
  bool refresh = false;
  for (uint32_t base = 0; base < n; base += 1024) {
    const uint32_t e = base + tid;
    bool end = false;
    float er = 0.0f;
    if (e < n) {
      er = ep_reward[e] + rewards[e];
      end = dones[e] || ep_steps[e] >= max_steps;
      ep_reward[e] = end ? 0.0f : er;
      reset_mask[e] = end ? 1 : 0;
    }
    s_er[tid] = er;
    s_end[tid] = end ? 1 : 0;
    __syncthreads();
    if (tid < 64) {
      for (int c = 0; c < 1024 && base + c < n; c += 64) {
        const float v0 = s_er[c + lane];
        unsigned long long bal = __ballot(s_end[c + lane] != 0);
        while (bal) {   // uniform loop: every lane tracks the same Book
          const int l = __builtin_ctzll(bal);
          bal &= bal - 1;
          const float v = __shfl(v0, l);
          if (b.hist_len < hist_cap) {
            if (lane == 0) hist[(b.hist_head + b.hist_len) % hist_cap] = v;
            b.hist_len += 1;
          } else {
            if (lane == 0) hist[b.hist_head] = v;
            b.hist_head = (b.hist_head + 1) % hist_cap;
          }
          refresh = refresh || b.episode_count >= hist_cap;
          b.episode_count += 1;
        }
      }
    }
    __syncthreads();
  }
  if (tid < 64) {
    if (refresh) {
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // lane 0's FIFO stores, before the other lanes read
      float s = 0.0f;
      for (uint32_t c = 0; c < b.hist_len; c += 64) {
        const float v = c + lane < b.hist_len ? hist[(b.hist_head + c + lane) % hist_cap] : 0.0f;
        const uint32_t m = b.hist_len - c < 64 ? b.hist_len - c : 64;
        for (uint32_t j = 0; j < m; ++j) s += __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), (int)j));
      }
      b.running_reward = s / (float)b.hist_len;
    }
    if (lane == 0) *book = b;
  }
}

std::vector<double> epsilon_table(const qlx_params& p) {
  std::vector<double> eps;
  double e = p.epsilon_max;
  const double delta = (p.epsilon_max - p.epsilon_min) / p.epsilon_greedy_steps;
  const size_t cap = 1u << 26;
  while (eps.size() < cap) {
    eps.push_back(e);
    if (e <= p.epsilon_min) break;
    e = std::max(e - delta, p.epsilon_min);
  }
  return eps;
}

void learner_book_stats(const EpisodeBooks& eb, float goal, float pct, float* running, uint64_t* solved) {
  *running = eb.book.running_reward;
  if (eb.rewards.empty()) { *solved = 0; return; }
  float mn = eb.rewards[0];
  for (float v : eb.rewards) mn = std::min(mn, v);
  *solved = (eb.book.running_reward >= goal && mn >= goal * pct) ? 1 : 0;
}

// ---- setup ----------------------------------------------------------------------------------------

void LearnerCore::validate(const qlx_params& p) {
  QLX_CHECK(p.n_envs > 0 && p.batch_size > 0 && p.batch_size <= 4096, QLX_E_INVALID, "bad n_envs / batch_size");
  QLX_CHECK(p.update_after_actions > 0 && p.history_buffer_len >= p.batch_size, QLX_E_INVALID, "bad parameters");
  QLX_CHECK(p.episode_reward_history_buffer_len > 0, QLX_E_INVALID, "episode_reward_history_buffer_len must be > 0");
  QLX_CHECK((p.flags & ~(QLX_LEARNER_DOUBLE_DQN | QLX_LEARNER_PER)) == 0, QLX_E_INVALID, "unknown learner flags");
  QLX_CHECK(!(p.flags & QLX_LEARNER_PER) || (std::isfinite(p.per_alpha) && std::isfinite(p.per_beta) && std::isfinite(p.per_eps) &&
                                             p.per_alpha >= 0.0f && p.per_beta >= 0.0f && p.per_eps > 0.0f),
            QLX_E_INVALID, "prioritized replay needs finite alpha >= 0, beta >= 0, eps > 0");
}

void LearnerCore::init(const qlx_params& params, int dev) {
  ddqn = (params.flags & QLX_LEARNER_DOUBLE_DQN) != 0;
  per = (params.flags & QLX_LEARNER_PER) != 0;
  p = params;
  device = dev;
  N = p.n_envs;
  B = p.batch_size;
  QLX_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  // epsilon table: eps_k after k decrements, k = 0.. until epsilon_min (repeated f64 subtraction)
  const std::vector<double> eps = epsilon_table(p);
  eps_len = eps.size();
  d_eps.alloc(eps.size());
  QLX_HIP(hipMemcpy(d_eps, eps.data(), eps.size() * sizeof(double), hipMemcpyHostToDevice));
  max_updates = (uint32_t)(N / p.update_after_actions + 2);
  d_actions.alloc(N);
  d_rewards.alloc(N);
  d_dones.alloc(N);
  d_reset.alloc(N);
  d_ep_reward.alloc(N);
  d_hist.alloc(p.episode_reward_history_buffer_len);
  d_book.alloc(1);
  const size_t UB = max_samples();
  d_idx.alloc(UB);
  d_bact.alloc(UB);
  d_brew.alloc(UB);
  d_bdone.alloc(UB);
  d_losses.alloc(max_updates);
  d_targets.alloc(UB);
  QLX_HIP(hipMemsetAsync(d_ep_reward, 0, N * sizeof(float), stream));
  QLX_HIP(hipMemsetAsync(d_book, 0, sizeof(Book), stream));
  QLX_HIP(hipMemsetAsync(d_actions, 0, N, stream));
  QLX_HIP(hipMemsetAsync(d_rewards, 0, N * sizeof(float), stream));
  QLX_HIP(hipMemsetAsync(d_dones, 0, N, stream));
  if (per) prio.init(p.history_buffer_len, UB);
}

// ---- the vector step ------------------------------------------------------------------------------

void LearnerCore::select_actions(const float* q, uint32_t n_actions, uint32_t id_offset, Profiler* prof) {
  ProfScope ps(prof, "select", stream);
  hipLaunchKernelGGL(k_select_actions, dim3((N + 255) / 256), dim3(256), 0, stream, N, n_actions, step_count,
                     p.epsilon_pure_random_steps, d_eps, eps_len, p.epsilon_min, p.learner_seed, id_offset, (uint32_t)vec_steps, q,
                     d_actions);
  QLX_HIP(hipGetLastError());
  step_count += N;
}

void LearnerCore::per_push(uint64_t cap, uint64_t first, Profiler* prof) {
  if (!per) return;
  ProfScope ps(prof, "per_push", stream);
  per_launch_push(stream, prio.leaves(), cap, first, N, prio.d_max);
}

void LearnerCore::episode_book(const uint32_t* ep_steps, const uint8_t* ended, uint8_t* reset_mask) {
  hipLaunchKernelGGL(k_episode_book, dim3(1), dim3(1024), 0, stream, N, d_rewards, ended, ep_steps, p.max_steps_per_episode,
                     d_ep_reward, d_hist, (uint32_t)p.episode_reward_history_buffer_len, d_book, reset_mask);
  QLX_HIP(hipGetLastError());
}

uint32_t LearnerCore::updates_due(uint64_t step_before, uint64_t replay_len) const {
  const uint64_t ua = p.update_after_actions;
  const uint64_t triggers = step_count / ua - step_before / ua;
  if (replay_len <= B || triggers == 0) return 0;
  QLX_CHECK(triggers <= max_updates, QLX_E_STATE, "too many updates per vector step");
  return (uint32_t)triggers;
}

void LearnerCore::sample(uint32_t U, uint64_t len, uint64_t cap, uint64_t start, Profiler* prof) {
  ProfScope ps(prof, "sample", stream);
  if (!per) {
    launch_sample_distinct(stream, p.learner_seed, (uint32_t)update_count, U, p.rank, len, B, d_idx);
    return;
  }
  {
    ProfScope pb(prof, "per_tree_build", stream);
    per_launch_build(stream, prio.d_tree, prio.L);
  }
  ProfScope pd(prof, "per_draw", stream);
  per_launch_sample(stream, prio.d_tree, prio.L, p.learner_seed, (uint32_t)update_count, U, p.rank, len, p.per_beta, B, cap, start,
                    d_idx, prio.d_w);
}

void LearnerCore::write_priorities(uint32_t U, uint64_t cap, uint64_t start, Profiler* prof) {
  if (!per) return;
  ProfScope ps(prof, "priorities", stream);
  per_launch_update(stream, d_idx, prio.d_td, U * B, cap, start, p.per_alpha, p.per_eps, prio.d_owner, prio.leaves(), prio.d_max);
}

void LearnerCore::record_metrics(const float* q, uint32_t n_actions, const float* d_norms, uint32_t n_vars, float clipnorm,
                                 const uint8_t* actions, const float* y, const float* weights, const float* loss, Profiler* prof) {
  if (!d_metrics) return;
  ProfScope ps(prof, "metrics", stream);
  MetricsArgs a{};
  a.q = q;
  a.actions = actions;
  a.y = y;
  a.weights = weights;
  a.loss = loss;
  a.norms = d_norms;
  a.B = B;
  a.n_actions = n_actions;
  a.n_vars = n_vars;
  a.clipnorm = clipnorm;
  a.update = update_count;
  a.step_count = step_count;
  a.row = d_metrics + metrics_recorded % d_metrics.size();
  launch_update_metrics(stream, a);
  metrics_recorded += 1;
}

// ---- the metrics ring -----------------------------------------------------------------------------

void LearnerCore::metrics_enable(uint32_t capacity) {
  QLX_CHECK(capacity <= kMetricsMaxRows, QLX_E_INVALID, "metrics capacity above 1 << 20 rows");
  QLX_HIP(hipSetDevice(device));
  QLX_HIP(hipStreamSynchronize(stream));   // an enqueued update may still write the old ring
  d_metrics.release();
  h_metrics.release();
  metrics_recorded = metrics_next = 0;
  if (!capacity) return;
  h_metrics.alloc(capacity);
  d_metrics.alloc(capacity);
}

// the oldest recorded update whose row a read can still return
static uint64_t metrics_first(const LearnerCore& c) {
  const uint64_t cap = c.d_metrics.size();
  return std::max(c.metrics_next, c.metrics_recorded - std::min(c.metrics_recorded, cap));
}

void LearnerCore::metrics_info(uint32_t* capacity, uint64_t* recorded, uint64_t* unread) const {
  QLX_CHECK(d_metrics, QLX_E_STATE, "metrics are off (qlx_learner_metrics_enable)");
  if (capacity) *capacity = (uint32_t)d_metrics.size();
  if (recorded) *recorded = metrics_recorded;
  if (unread) *unread = metrics_recorded - metrics_first(*this);
}

void LearnerCore::metrics_read(qlx_update_metrics* out, uint64_t cap, uint64_t* n, uint64_t* dropped) {
  QLX_CHECK(d_metrics, QLX_E_STATE, "metrics are off (qlx_learner_metrics_enable)");
  QLX_HIP(hipSetDevice(device));
  const uint64_t ring = d_metrics.size(), first = metrics_first(*this);
  const uint64_t m = std::min(cap, metrics_recorded - first);
  // slots first % ring .. in ring order: one copy, or two where the rows wrap
  const uint64_t s0 = first % ring, m0 = std::min(m, ring - s0);
  if (m0) QLX_HIP(hipMemcpyAsync(h_metrics, d_metrics + s0, m0 * sizeof(qlx_update_metrics), hipMemcpyDeviceToHost, stream));
  if (m > m0)
    QLX_HIP(hipMemcpyAsync(h_metrics + m0, d_metrics, (m - m0) * sizeof(qlx_update_metrics), hipMemcpyDeviceToHost, stream));
  QLX_HIP(hipStreamSynchronize(stream));
  std::copy(h_metrics.get(), h_metrics.get() + m, out);
  *n = m;
  *dropped = first - metrics_next;
  metrics_next = first + m;
}

// ---- read-outs ------------------------------------------------------------------------------------

EpisodeBooks LearnerCore::books() {
  QLX_HIP(hipStreamSynchronize(stream));
  EpisodeBooks eb;
  QLX_HIP(hipMemcpy(&eb.book, d_book, sizeof(Book), hipMemcpyDeviceToHost));
  const Book& b = eb.book;
  if (b.hist_len == 0) return eb;
  std::vector<float> ring(p.episode_reward_history_buffer_len);
  QLX_HIP(hipMemcpy(ring.data(), d_hist, ring.size() * sizeof(float), hipMemcpyDeviceToHost));
  eb.rewards.resize(b.hist_len);
  for (uint32_t i = 0; i < b.hist_len; ++i) eb.rewards[i] = ring[(b.hist_head + i) % ring.size()];
  return eb;
}

void LearnerCore::stats(float goal, uint64_t replay_len, qlx_learner_stats* out) {
  const EpisodeBooks eb = books();
  out->step_count = step_count;
  out->vec_steps = vec_steps;
  out->update_count = update_count;
  out->episode_count = eb.book.episode_count;
  out->replay_len = replay_len;
  // epsilon after step_count decrements
  double e = p.epsilon_min;
  if (step_count < eps_len) QLX_HIP(hipMemcpy(&e, d_eps + step_count, sizeof(double), hipMemcpyDeviceToHost));
  out->epsilon = e;
  learner_book_stats(eb, goal, p.lowest_episode_reward_goal_threshold_pct, &out->running_reward, &out->solved);
  float loss = 0.0f;
  if (last_updates) QLX_HIP(hipMemcpy(&loss, d_losses + last_updates - 1, sizeof(float), hipMemcpyDeviceToHost));
  out->last_loss = loss;
}

void LearnerCore::last(uint8_t* actions, float* rewards, uint8_t* dones, float* losses, uint64_t* indices, float* targets,
                       uint32_t* n_updates) {
  QLX_HIP(hipStreamSynchronize(stream));
  const uint32_t U = last_updates;
  if (actions) QLX_HIP(hipMemcpy(actions, d_actions, N, hipMemcpyDeviceToHost));
  if (rewards) QLX_HIP(hipMemcpy(rewards, d_rewards, N * sizeof(float), hipMemcpyDeviceToHost));
  if (dones) QLX_HIP(hipMemcpy(dones, d_dones, N, hipMemcpyDeviceToHost));
  if (U && losses) QLX_HIP(hipMemcpy(losses, d_losses, U * sizeof(float), hipMemcpyDeviceToHost));
  if (U && indices) QLX_HIP(hipMemcpy(indices, d_idx, (size_t)U * B * 8, hipMemcpyDeviceToHost));
  if (U && targets) QLX_HIP(hipMemcpy(targets, d_targets, (size_t)U * B * 4, hipMemcpyDeviceToHost));
  if (n_updates) *n_updates = U;
}

void LearnerCore::priorities(float* is_weights, float* leaves, float* per_max) {
  QLX_HIP(hipStreamSynchronize(stream));
  const uint32_t U = last_updates;
  if (U && is_weights) QLX_HIP(hipMemcpy(is_weights, prio.d_w, (size_t)U * B * 4, hipMemcpyDeviceToHost));
  if (leaves) QLX_HIP(hipMemcpy(leaves, prio.leaves(), prio.cap * 4, hipMemcpyDeviceToHost));
  if (per_max) QLX_HIP(hipMemcpy(per_max, prio.d_max, 4, hipMemcpyDeviceToHost));
}

void LearnerCore::episode_rewards(float* out, uint64_t cap, uint64_t* n) {
  const std::vector<float> r = books().rewards;
  if (n) *n = r.size();
  if (out) std::copy(r.begin(), r.begin() + std::min<uint64_t>(cap, r.size()), out);
}

void LearnerCore::action_counts(const uint8_t* d_replay_actions, uint64_t replay_len, uint32_t n_actions, uint64_t* counts) {
  std::vector<uint64_t> c;
  qlx::action_counts(stream, d_replay_actions, replay_len, n_actions, c);
  std::copy(c.begin(), c.end(), counts);
}

// learning statistics (learning_update_log, self_driving_tf_q_learner.rs:235-273; stats.hip)
std::string LearnerCore::update_log(float goal, const char* const* action_names, uint32_t n_actions,
                                    const uint8_t* d_replay_actions, uint64_t replay_len) {
  qlx_learner_stats st;
  stats(goal, replay_len, &st);
  LogInputs in{st.episode_count, st.step_count, p.gamma, st.epsilon, goal, p.lowest_episode_reward_goal_threshold_pct,
               books().rewards, {}, action_names};
  qlx::action_counts(stream, d_replay_actions, replay_len, n_actions, in.counts);
  return learning_log(in);
}

}  // namespace qlx
