// The Breakout learner object (internal): the shared core plus env, replay, the two Q-nets, the data-parallel state and
// the Bellman-target memo.  Steps and C API: learner.hip; save / load: learner_snapshot.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <rccl/rccl.h>

#include <string>

#include "learner_core.h"
#include "objects.h"
#include "profiler.h"

struct qlx_learner : qlx::LearnerCore {
  qlx_env* env = nullptr;
  qlx_replay* rb = nullptr;
  qlx_model* online = nullptr;
  qlx_model* target = nullptr;
  // device buffers
  qlx::DeviceBuffer<const uint8_t*> d_obs_table;
  qlx::DeviceBuffer<const uint8_t*> d_tab_s, d_tab_sn;   // [max_updates][B][4] frame pointers of s / s'
  // data parallel
  ncclComm_t comm = nullptr;
  hipStream_t comm_stream = nullptr;   // the communicator's collectives (bucketed gradient all-reduce)
  bool dp_overlap = true;              // QLX_DP_OVERLAP=0: one whole-gradient all-reduce after the backward
  bool dp_fold = true;                 // fp32 dense norm partials in the conv backward's reduction launch (QLX_DP_FOLD=0:
                                       // a launch of their own on the communicator stream)
  hipEvent_t ev_dense = nullptr, ev_reduced = nullptr;
  int world = 1, rank = 0;
  // global solved() over ranks: per vector step, {sum running_reward, sum has_history, sum episodes} (f64) and {min
  // episode reward} all-reduced on the learner stream (d_gsum[3], d_gmin[1])
  qlx::DeviceBuffer<double> d_gsum;
  qlx::DeviceBuffer<float> d_gmin;
  // pinned host copies read after every vector step (the solved() check): Book + the global sums
  qlx::PinnedBuffer<qlx::Book> h_book;
  qlx::PinnedBuffer<double> h_gsum;
  // frame_sparsity's counters: a device buffer and its pinned host copy (8 x u64: the train and the acting halves)
  qlx::DeviceBuffer<unsigned long long> d_sparsity;
  qlx::PinnedBuffer<unsigned long long> h_sparsity;
  // Bellman-target memo per replay slot (ycache_fill): on when the target net is frozen (target_sync_steps == 0,
  // the reference) and y does not depend on the online net (no double DQN); QLX_TARGET_CACHE=0 turns it off
  bool ycache = false;
  qlx::DeviceBuffer<float> d_ycache;           // [capacity] y of the transition in each ring slot
  qlx::DeviceBuffer<const uint8_t*> d_ytab;    // [ychunk * 4]
  qlx::DeviceBuffer<float> d_yrew, d_ytmp;     // [ychunk]
  qlx::DeviceBuffer<uint8_t> d_ydone;          // [ychunk]
  uint32_t ychunk = 0;
  uint64_t ycache_version = 0;         // target->version the memo was computed with
  // n-step returns (qlx_params.n_step > 1).  The memo then holds the bootstrap value v = max_a Q_target(s')
  // per slot instead of y, and every target pass runs the head with gamma = 1 over zero rewards / dones (d_zero: zero
  // bytes, read as both) so that it leaves v; R, g and terminal of the sampled windows are kept only without the memo.
  uint32_t n_step = 1;
  qlx::DeviceBuffer<float> d_zero;             // zeros (zero_reserve)
  qlx::DeviceBuffer<float> d_nret;             // [max_updates][B] R
  qlx::DeviceBuffer<float> d_ndisc;            // [max_updates][B] g = gamma^m
  qlx::DeviceBuffer<uint8_t> d_nterm;          // [max_updates][B] done of the window's last transition
  qlx::Profiler prof;
  // statistics events (write_checkpoint + learning_update_log, self_driving_tf_q_learner.rs:204-212,226-230)
  uint64_t stats_events = 0;
  uint64_t seen_episodes = 0;
  std::string last_log;
  void (*log_cb)(const char*, void*) = nullptr;
  void* log_user = nullptr;
};
