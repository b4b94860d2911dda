// The environment-independent half of a learner (learner_core.hip): parameters and counters, epsilon-greedy acting,
// episode bookkeeping, the update trigger, replay sampling (uniform or prioritized), the priority write-back and the
// read-outs of the C API.  qlx_learner (Breakout, learner.h) and qlx_bg_learner (BallGame, ballgame.hip) are this
// struct plus their env, replay and models, and call its functions with what differs between them as arguments.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "per.h"
#include "qlx_internal.h"

namespace qlx {

struct Profiler;

// episode bookkeeping state of a learner (k_episode_book)
struct Book {
  uint64_t episode_count;
  float running_reward;
  uint32_t hist_len;     // current entries in the episode reward ring
  uint32_t hist_head;    // index of the oldest entry
};

// the Book and the episode reward history, oldest first, as of now
struct EpisodeBooks {
  Book book;
  std::vector<float> rewards;
};

// epsilon after k decrements, k = 0 .. until epsilon_min (repeated f64 subtraction, learn_episode :164-167)
std::vector<double> epsilon_table(const qlx_params& p);
// solved() over the episode reward history (self_driving_tf_q_learner.rs:134-139)
void learner_book_stats(const EpisodeBooks& eb, float goal, float pct, float* running, uint64_t* solved);

struct LearnerCore {
  qlx_params p{};
  int device = 0;
  hipStream_t stream = nullptr;    // created by init, destroyed by the learner once its env, replay and models are gone
  uint32_t N = 0, B = 0, max_updates = 0;
  bool ddqn = false, per = false;  // qlx_params.flags
  PerState prio;                   // prioritized replay (per.hip)
  // host counters
  uint64_t step_count = 0, vec_steps = 0, update_count = 0;
  uint32_t last_updates = 0;
  // per vector step
  DeviceBuffer<uint8_t> d_actions, d_dones, d_reset;
  DeviceBuffer<float> d_rewards;
  DeviceBuffer<double> d_eps;
  uint64_t eps_len = 0;
  DeviceBuffer<float> d_ep_reward, d_hist;
  DeviceBuffer<Book> d_book;
  // the batches of one vector step
  DeviceBuffer<uint64_t> d_idx;       // [max_updates][B]
  DeviceBuffer<uint8_t> d_bact, d_bdone;
  DeviceBuffer<float> d_brew;
  DeviceBuffer<float> d_targets;      // [max_updates][B]
  DeviceBuffer<float> d_losses;       // [max_updates]
  // training metrics (metrics.hip; off unless metrics_enable allocated the ring): the row of the r-th recorded update is
  // in slot r % capacity; the host has consumed (read or counted as dropped) the first metrics_next of them
  DeviceBuffer<qlx_update_metrics> d_metrics;   // [capacity]
  PinnedBuffer<qlx_update_metrics> h_metrics;   // [capacity] staging of metrics_read
  uint64_t metrics_recorded = 0, metrics_next = 0;

  // ---- setup
  // the parameter checks both learners share (p non-null); each learner adds its own
  static void validate(const qlx_params& p);
  // flags, the stream, the epsilon table, every buffer above (zeroed where the first step reads it) and the sum tree
  void init(const qlx_params& p, int device);
  size_t max_samples() const { return (size_t)max_updates * B; }   // all batches of one vector step

  // ---- one vector step, in this order (every launch on `stream`; `prof` may be null)
  // epsilon-greedy actions of the N envs (global ids id_offset + e) from q [N][n_actions] into d_actions; advances
  // step_count by N
  void select_actions(const float* q, uint32_t n_actions, uint32_t id_offset, Profiler* prof = nullptr);
  // prioritized replay: the N transitions pushed at ring positions first .. first + N - 1 (first = the total before the
  // push) enter with the largest priority so far
  void per_push(uint64_t cap, uint64_t first, Profiler* prof = nullptr);
  // d_rewards / `ended` (or max_steps_per_episode) into the episode reward sums, the reward FIFO and the Book; marks the
  // envs to reset in `reset_mask`
  void episode_book(const uint32_t* ep_steps, const uint8_t* ended, uint8_t* reset_mask);
  void episode_book(const uint32_t* ep_steps) { episode_book(ep_steps, d_dones, d_reset); }
  // updates this vector step owes (it began at step_before): 0 while the replay holds no more than B transitions
  uint32_t updates_due(uint64_t step_before, uint64_t replay_len) const;
  // logical replay indices of U batches into d_idx (prioritized: + IS weights into prio.d_w); start = ring slot of the
  // oldest transition
  void sample(uint32_t U, uint64_t len, uint64_t cap, uint64_t start, Profiler* prof = nullptr);
  // prioritized replay: |TD error| of the U batches (prio.d_td) into the leaves
  void write_priorities(uint32_t U, uint64_t cap, uint64_t start, Profiler* prof = nullptr);
  bool target_sync_due(uint64_t step_before) const {
    const uint64_t ts = p.target_sync_steps;
    return ts > 0 && step_count / ts != step_before / ts;
  }
  // training metrics of the update being enqueued, into the ring's next slot: called after the update's Adam (d_norms is
  // final) and before update_count advances; q [B][n_actions] is what the training head wrote, actions / y / weights
  // (null without prioritized replay) / loss are the update's.  With metrics off it returns before touching the device.
  void record_metrics(const float* q, uint32_t n_actions, const float* d_norms, uint32_t n_vars, float clipnorm,
                      const uint8_t* actions, const float* y, const float* weights, const float* loss, Profiler* prof = nullptr);

  // ---- read-outs (each synchronises the stream); the arguments are what the two environments differ in
  EpisodeBooks books();
  void stats(float goal, uint64_t replay_len, qlx_learner_stats* out);
  void last(uint8_t* actions, float* rewards, uint8_t* dones, float* losses, uint64_t* indices, float* targets, uint32_t* n_updates);
  void priorities(float* is_weights, float* leaves, float* per_max);
  void episode_rewards(float* out, uint64_t cap, uint64_t* n);
  void action_counts(const uint8_t* d_replay_actions, uint64_t replay_len, uint32_t n_actions, uint64_t* counts);
  std::string update_log(float goal, const char* const* action_names, uint32_t n_actions, const uint8_t* d_replay_actions,
                         uint64_t replay_len);
  // the metrics ring (qlx_learner_metrics_enable / _info / _read); enable and read synchronise the stream
  void metrics_enable(uint32_t capacity);
  void metrics_info(uint32_t* capacity, uint64_t* recorded, uint64_t* unread) const;
  void metrics_read(qlx_update_metrics* out, uint64_t cap, uint64_t* n, uint64_t* dropped);
};

}  // namespace qlx
