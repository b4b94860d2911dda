// Policy evaluation on one MI355X (beyond the reference; DESIGN.md "Policy evaluation"): n_envs fresh Breakout envs play
// K episodes each with a model's current weights, greedily or at a fixed epsilon.  The loop composes the batched env,
// the model's own forward + head and the Philox streams like the learner's acting branch (learner.hip
// k_select_actions; self_driving_tf_q_learner.rs:153-167), with two kernels of its own:
//   k_eval_select  argmax / max-Q / epsilon draw per row of the active list, the action scattered to its env
//   k_eval_book    episode records per env, then the stable (env-order) list of the envs still playing and the frame
//                  pointer table [B][4] of the next forward
// Episodes end at very different times, so the forward runs over B rows = the active count the host read at its last
// poll (every poll_steps vector steps: one pinned 8-byte copy, an event and a wait); nothing else synchronises.
// A run on a model's wide head (qlx_evaluator_run_head) is the same loop with the step "Q and select"
// exchanged: the head's forward into the evaluator's Z rows, then dist_loss.hip's k_dist_select in place of the built-in
// head and k_eval_select.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

#include "dist_loss.h"
#include "head_wide.h"
#include "objects.h"
#include "qnet.h"

namespace qlx {

constexpr uint32_t kEvalPollDefault = 8;   // qlx_eval_config.poll_steps = 0 (DESIGN.md "Policy evaluation": measured)

// d_count: [0] envs still playing (what the host polls), [1] valid rows of the list (= [0] with compaction, n without)

__global__ __launch_bounds__(256) void k_eval_init(uint32_t n, const uint8_t* obs, uint32_t* list, const uint8_t** table,
                                                   float* ret, float* qsum, float* qmax, uint32_t* kdone, uint8_t* actions,
                                                   unsigned long long* counts, uint32_t* count) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  list[e] = e;
  for (int j = 0; j < kSlots; ++j) table[(size_t)e * kSlots + j] = obs + ((size_t)e * kSlots + j) * kFramePix;
  ret[e] = 0.0f;
  qsum[e] = 0.0f;
  qmax[e] = 0.0f;
  kdone[e] = 0;
  actions[e] = 0;
  if (e == 0) {
    for (int j = 0; j < kActions; ++j) counts[j] = 0;
    count[0] = n;
    count[1] = n;
  }
}

// Row r of the forward = env list[r].  Draws as k_select_actions lays them out (f64 from words 0-1, the random action
// from word 2 on) under a purpose of their own, so evaluation shares no words with training.  Rows past the list, and
// (without compaction) rows of retired envs, leave nothing behind.
__global__ __launch_bounds__(256) void k_eval_select(uint32_t rows, const uint32_t* count, const uint32_t* list, const float* q,
                                                     uint32_t K, const uint32_t* kdone, double epsilon, uint64_t seed, uint32_t t,
                                                     uint8_t* actions, float* qmax, unsigned long long* counts) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  bool valid = r < rows && r < count[1];
  const uint32_t e = valid ? list[r] : 0;
  valid = valid && kdone[e] < K;
  uint32_t a = 0;
  if (valid) {
    uint32_t best = 0;   // tf.argmax over Q(s): first maximal index
    float bv = q[(size_t)r * kActions];
    for (uint32_t j = 1; j < (uint32_t)kActions; ++j)
      if (q[(size_t)r * kActions + j] > bv) { best = j; bv = q[(size_t)r * kActions + j]; }
    bool random = false;
    if (epsilon > 0.0) {
      RngStream su(seed, e, t, P_EVAL, 0);
      random = epsilon > uniform_f64_01(su);
    }
    if (random) {
      RngStream sa(seed, e, t, P_EVAL, 2);
      a = uniform_u8(sa, kActions);
    } else {
      a = best;
    }
    actions[e] = (uint8_t)a;
    qmax[e] = bv;
  }
  for (uint32_t j = 0; j < (uint32_t)kActions; ++j) {   // integer counts: one atomic per wave and action
    const unsigned long long bal = __ballot(valid && a == j);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(counts + j, (unsigned long long)__builtin_popcountll(bal));
  }
}

// One workgroup over all envs, 1024 per round (k_episode_book's shape).  Per env: the step's reward and max-Q join the
// running episode (fp32, step order); an episode that ended (done, or max_steps steps) is recorded at [e][k] and the
// env is marked for reset; an env with K records is retired: it keeps being stepped with action 0 and reset when it
// ends, nothing of it is counted.  Then the envs still playing, in env order: a ballot per wave, the waves' counts
// through LDS, a running offset over the rounds.  compact: they become the list and the frame table of the next
// forward; rows from the new count up to `rows` (what the host still launches) point at the list's first env (env 0
// when the list is empty).
__global__ __launch_bounds__(1024) void k_eval_book(uint32_t n, uint32_t K, const float* rewards, const uint8_t* dones,
                                                    const uint32_t* ep_steps, uint64_t max_steps, const float* qmax, float* ret,
                                                    float* qsum, uint32_t* kdone, float* rec_ret, uint32_t* rec_len, uint8_t* rec_term,
                                                    float* rec_qsum, uint8_t* reset_mask, uint8_t* actions, int compact, uint32_t rows,
                                                    const uint8_t* obs, uint32_t* list, const uint8_t** table, uint32_t* count) {
  __shared__ uint32_t s_wave[16];
  __shared__ uint32_t s_first;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) s_first = 0;
  uint32_t offset = 0;   // envs still playing before this round (uniform)
  for (uint32_t base = 0; base < n; base += 1024) {
    const uint32_t e = base + tid;
    bool alive = false;
    if (e < n) {
      uint32_t k = kdone[e];
      const uint32_t len = ep_steps[e];
      const bool done = dones[e] != 0;
      const bool end = done || len >= max_steps;
      if (k < K) {
        float r = ret[e] + rewards[e];
        float qs = qsum[e] + qmax[e];
        if (end) {
          const size_t i = (size_t)e * K + k;
          rec_ret[i] = r;
          rec_len[i] = len;
          rec_term[i] = done ? 1 : 0;
          rec_qsum[i] = qs;
          r = 0.0f;
          qs = 0.0f;
          k += 1;
          kdone[e] = k;
        }
        ret[e] = r;
        qsum[e] = qs;
      }
      reset_mask[e] = end ? 1 : 0;
      alive = k < K;
      if (!alive) actions[e] = 0;
    }
    const unsigned long long bal = __ballot(alive);
    if (lane == 0) s_wave[wave] = (uint32_t)__builtin_popcountll(bal);
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t w = 0; w < 16; ++w) {
      const uint32_t c = s_wave[w];
      before += w < wave ? c : 0;
      total += c;
    }
    if (alive && compact) {
      const uint32_t pos = offset + before + (uint32_t)__builtin_popcountll(bal & ((1ull << lane) - 1ull));
      list[pos] = e;
      for (int j = 0; j < kSlots; ++j) table[(size_t)pos * kSlots + j] = obs + ((size_t)e * kSlots + j) * kFramePix;
      if (pos == 0) s_first = e;
    }
    offset += total;
    __syncthreads();
  }
  if (compact) {
    const uint32_t first = s_first;
    for (uint32_t r = offset + tid; r < rows; r += 1024)
      for (int j = 0; j < kSlots; ++j) table[(size_t)r * kSlots + j] = obs + ((size_t)first * kSlots + j) * kFramePix;
  }
  if (tid == 0) {
    count[0] = offset;
    count[1] = compact ? offset : n;
  }
}

// the field a config is refused for (nullptr: the config is valid); no device is touched
static const char* eval_config_error(const qlx_eval_config& c) {
  if (c.n_envs < 1 || c.n_envs > QLX_EVAL_MAX_ENVS) return "n_envs must be 1..QLX_EVAL_MAX_ENVS";
  if (c.episodes_per_env < 1) return "episodes_per_env must be >= 1";
  if ((uint64_t)c.n_envs * c.episodes_per_env > (1ull << 24)) return "n_envs * episodes_per_env must be <= 1 << 24";
  if (c.max_steps_per_episode < 1) return "max_steps_per_episode must be >= 1";
  if (!(std::isfinite(c.epsilon) && c.epsilon >= 0.0 && c.epsilon <= 1.0)) return "epsilon must be finite and in 0..1";
  if (c.flags != 0) return "flags must be 0";
  return nullptr;
}

}  // namespace qlx

struct qlx_evaluator {
  qlx_eval_config cfg{};
  int device = 0;
  bool compact = true;   // QLX_EVAL_COMPACT=0: every step forwards all n_envs
  uint32_t poll = 0;
  qlx_env* env = nullptr;
  hipStream_t env_stream = nullptr;   // the env's own stream (it adopts the model's for a run)
  qlx::DeviceBuffer<uint8_t> d_actions, d_dones, d_reset;
  qlx::DeviceBuffer<float> d_rewards;
  qlx::DeviceBuffer<uint32_t> d_list;          // [n] envs still playing, env order
  qlx::DeviceBuffer<const uint8_t*> d_table;   // [n][4] frame pointers of the next forward
  qlx::DeviceBuffer<float> d_ret;              // [n] running episode return
  qlx::DeviceBuffer<float> d_qsum;             // [n] running sum of max_a q
  qlx::DeviceBuffer<float> d_qmax;             // [n] max_a q of the step being taken
  qlx::DeviceBuffer<uint32_t> d_kdone;         // [n] episodes recorded
  qlx::DeviceBuffer<float> d_rec_ret, d_rec_qsum;   // [n][K] records
  qlx::DeviceBuffer<uint32_t> d_rec_len;
  qlx::DeviceBuffer<uint8_t> d_rec_term;
  qlx::DeviceBuffer<unsigned long long> d_counts;   // [3] actions taken
  qlx::DeviceBuffer<uint32_t> d_count;              // [2] (k_eval_init)
  // a run on a wide head: its outputs over the forward's rows [n][width], grown only, before the loop of the first run that
  // needs it; fused_select = false (QLX_EVAL_HEAD_FUSED=0, the measurement's other arm): k_dist_values into d_hq [n][3],
  // then k_eval_select
  qlx::DeviceBuffer<float> d_z, d_hq;
  size_t z_floats = 0;
  bool fused_select = true;
  qlx::PinnedBuffer<uint32_t> h_count;              // pinned copy read at each poll
  hipEvent_t polled = nullptr;
  // host copies of the last run's records
  bool has_run = false;
  std::vector<float> rec_ret, rec_qsum;
  std::vector<uint32_t> rec_len;
  std::vector<uint8_t> rec_term;
};

namespace qlx {

// the run borrows the model: its profiler pointer and the env's stream go back however the run ends
struct EvalBorrow {
  qlx_evaluator* ev;
  qlx_model* m;
  Profiler* prof;
  EvalBorrow(qlx_evaluator* ev_, qlx_model* m_) : ev(ev_), m(m_), prof(m_->prof) {
    m->prof = nullptr;
    ev->env->stream = m->stream;
  }
  ~EvalBorrow() {
    (void)hipStreamSynchronize(m->stream);   // (a run that failed part-way: nothing of it is left in flight)
    m->prof = prof;
    ev->env->stream = ev->env_stream;
  }
};

static void launch_eval_select(qlx_evaluator* ev, uint32_t B, const float* q, uint32_t t, hipStream_t s) {
  const qlx_eval_config& c = ev->cfg;
  hipLaunchKernelGGL(k_eval_select, dim3((B + 255) / 256), dim3(256), 0, s, B, ev->d_count, ev->d_list, q, c.episodes_per_env,
                     ev->d_kdone, c.epsilon, c.policy_seed, t, ev->d_actions, ev->d_qmax, ev->d_counts);
  QLX_HIP(hipGetLastError());
}

// "Q and select" of the built-in head: after the trunk forward over B rows, row r's action into d_actions[list[r]], its
// max-Q into d_qmax, the action counts
struct SelectBuiltin {
  void prepare(qlx_evaluator*, qlx_model*) const {}
  void operator()(qlx_evaluator* ev, qlx_model* m, uint32_t B, uint32_t t, hipStream_t s) const {
    Fc2Args a = fc2_args(m, (int)B);
    model_head(m, 0, a, (int)B, s);
    launch_eval_select(ev, B, m->w.q, t, s);
  }
};

// ... of a wide head read as `d`: no built-in head launch
struct SelectHead {
  qlx_head* h;
  qlx_dist d;
  void prepare(qlx_evaluator* ev, qlx_model*) const {
    const size_t need = (size_t)ev->cfg.n_envs * (size_t)h->width;
    if (need > ev->z_floats) {
      ev->d_z.release();
      ev->z_floats = 0;
      ev->d_z.alloc(need);
      ev->z_floats = need;
    }
    if (!ev->fused_select && !ev->d_hq) ev->d_hq.alloc((size_t)ev->cfg.n_envs * kActions);
  }
  void operator()(qlx_evaluator* ev, qlx_model*, uint32_t B, uint32_t t, hipStream_t s) const {
    const qlx_eval_config& c = ev->cfg;
    head_forward_launch(h, B, ev->d_z, s);
    if (ev->fused_select) {
      const DistSelectRows rows{ev->d_list, ev->d_count, ev->d_kdone, c.episodes_per_env, ev->d_counts};
      dist_select(d, ev->d_z, B, &rows, c.epsilon, c.policy_seed, t, P_EVAL, ev->d_actions, ev->d_qmax, nullptr, s);
    } else {
      dist_values(d, ev->d_z, B, ev->d_hq, nullptr, nullptr, s);
      launch_eval_select(ev, B, ev->d_hq, t, s);
    }
  }
};

template <class Select>
static void evaluator_run(qlx_evaluator* ev, qlx_model* m, const Select& select, qlx_eval_summary* out) {
  const qlx_eval_config& c = ev->cfg;
  const uint32_t n = c.n_envs, K = c.episodes_per_env, P = ev->poll;
  QLX_HIP(hipSetDevice(ev->device));
  model_workspace(m, (int)n);
  select.prepare(ev, m);
  EvalBorrow borrow(ev, m);
  hipStream_t s = m->stream;
  qlx_env* env = ev->env;
  env_launch_reset(env, nullptr, 0);
  hipLaunchKernelGGL(k_eval_init, dim3((n + 255) / 256), dim3(256), 0, s, n, env->d_obs, ev->d_list, ev->d_table, ev->d_ret,
                     ev->d_qsum, ev->d_qmax, ev->d_kdone, ev->d_actions, ev->d_counts, ev->d_count);
  QLX_HIP(hipGetLastError());
  debug_sync(s, "eval init");
  // every episode is over after max_steps steps, so no env plays past K * max_steps vector steps
  const uint64_t bound = c.max_steps_per_episode > UINT64_MAX / K ? UINT64_MAX : c.max_steps_per_episode * K;
  uint64_t t = 0, forward_samples = 0;
  uint32_t B = n;   // rows of the forward: the active count of the last poll
  for (;;) {
    for (uint32_t i = 0; i < P; ++i, ++t) {
      model_forward_trunk(m, ev->d_table, (int)B, s, false);
      select(ev, m, B, (uint32_t)t, s);
      debug_sync(s, "eval act + select");
      env_launch_step(env, ev->d_actions, ev->d_rewards, ev->d_dones);
      hipLaunchKernelGGL(k_eval_book, dim3(1), dim3(1024), 0, s, n, K, ev->d_rewards, ev->d_dones, env->d_ep_steps,
                         c.max_steps_per_episode, ev->d_qmax, ev->d_ret, ev->d_qsum, ev->d_kdone, ev->d_rec_ret, ev->d_rec_len,
                         ev->d_rec_term, ev->d_rec_qsum, ev->d_reset, ev->d_actions, ev->compact ? 1 : 0, B, env->d_obs, ev->d_list,
                         ev->d_table, ev->d_count);
      QLX_HIP(hipGetLastError());
      env_launch_reset(env, ev->d_reset, 1);
      debug_sync(s, "eval env step + book");
      forward_samples += B;
    }
    QLX_HIP(hipMemcpyAsync(ev->h_count, ev->d_count, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    QLX_HIP(hipEventRecord(ev->polled, s));
    QLX_HIP(hipEventSynchronize(ev->polled));
    const uint32_t active = ev->h_count[0];
    if (active == 0) break;
    QLX_CHECK(t < bound, QLX_E_STATE, "evaluation: envs still playing after episodes_per_env * max_steps_per_episode steps");
    if (ev->compact) B = active;
  }
  const size_t R = (size_t)n * K;
  unsigned long long counts[kActions];
  QLX_HIP(hipMemcpyAsync(ev->rec_ret.data(), ev->d_rec_ret, R * sizeof(float), hipMemcpyDeviceToHost, s));
  QLX_HIP(hipMemcpyAsync(ev->rec_len.data(), ev->d_rec_len, R * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  QLX_HIP(hipMemcpyAsync(ev->rec_term.data(), ev->d_rec_term, R, hipMemcpyDeviceToHost, s));
  QLX_HIP(hipMemcpyAsync(ev->rec_qsum.data(), ev->d_rec_qsum, R * sizeof(float), hipMemcpyDeviceToHost, s));
  QLX_HIP(hipMemcpyAsync(counts, ev->d_counts, sizeof(counts), hipMemcpyDeviceToHost, s));
  QLX_HIP(hipStreamSynchronize(s));
  ev->has_run = true;
  // sums on the host in double over the records in [e][k] order
  qlx_eval_summary sm{};
  double sum_ret = 0.0, sum_q = 0.0;
  float mn = ev->rec_ret[0], mx = ev->rec_ret[0];
  for (size_t i = 0; i < R; ++i) {
    sum_ret += (double)ev->rec_ret[i];
    sum_q += (double)ev->rec_qsum[i];
    sm.env_steps += ev->rec_len[i];
    sm.terminal_episodes += ev->rec_term[i];
    mn = std::min(mn, ev->rec_ret[i]);
    mx = std::max(mx, ev->rec_ret[i]);
  }
  sm.episodes = R;
  sm.vector_steps = t;
  sm.forward_samples = forward_samples;
  for (int j = 0; j < kActions; ++j) sm.action_counts[j] = counts[j];
  sm.mean_return = sum_ret / (double)R;
  sm.mean_length = (double)sm.env_steps / (double)R;
  sm.mean_max_q = sum_q / (double)sm.env_steps;
  sm.min_return = mn;
  sm.max_return = mx;
  *out = sm;
}

}  // namespace qlx

using namespace qlx;

extern "C" {

int32_t qlx_evaluator_create(const qlx_eval_config* cfg, int32_t device, qlx_evaluator** out) {
  return guard([&] {
    QLX_CHECK(cfg && out, QLX_E_INVALID, "null argument");
    const char* bad = eval_config_error(*cfg);
    QLX_CHECK(!bad, QLX_E_INVALID, std::string("qlx_eval_config: ") + bad);
    current_device_checked(device);
    auto* ev = new qlx_evaluator;
    try {   // a failure part-way releases what was built
      ev->cfg = *cfg;
      ev->device = device;
      ev->poll = cfg->poll_steps ? cfg->poll_steps : kEvalPollDefault;
      const char* sw = std::getenv("QLX_EVAL_COMPACT");
      ev->compact = !(sw && sw[0] == '0');
      const char* fs = std::getenv("QLX_EVAL_HEAD_FUSED");
      ev->fused_select = !(fs && fs[0] == '0');
      const uint32_t n = cfg->n_envs;
      const size_t R = (size_t)n * cfg->episodes_per_env;
      const int32_t st = qlx_env_create(QLX_ENV_BREAKOUT, n, cfg->env_seed, device, &ev->env);
      QLX_CHECK(st == QLX_OK, st, qlx_last_error());
      ev->env_stream = ev->env->stream;
      ev->env->hashing = false;
      ev->d_actions.alloc(n);
      ev->d_rewards.alloc(n);
      ev->d_dones.alloc(n);
      ev->d_reset.alloc(n);
      ev->d_list.alloc(n);
      ev->d_table.alloc((size_t)n * kSlots);
      ev->d_ret.alloc(n);
      ev->d_qsum.alloc(n);
      ev->d_qmax.alloc(n);
      ev->d_kdone.alloc(n);
      ev->d_rec_ret.alloc(R);
      ev->d_rec_len.alloc(R);
      ev->d_rec_term.alloc(R);
      ev->d_rec_qsum.alloc(R);
      ev->d_counts.alloc(kActions);
      ev->d_count.alloc(2);
      ev->h_count.alloc(2);
      QLX_HIP(hipEventCreateWithFlags(&ev->polled, hipEventDisableTiming));
      ev->rec_ret.resize(R);
      ev->rec_qsum.resize(R);
      ev->rec_len.resize(R);
      ev->rec_term.resize(R);
    } catch (...) {
      qlx_evaluator_destroy(ev);
      throw;
    }
    *out = ev;
  });
}

int32_t qlx_evaluator_destroy(qlx_evaluator* ev) {
  return guard([&] {
    if (!ev) return;
    (void)hipSetDevice(ev->device);
    qlx_env_destroy(ev->env);
    if (ev->polled) (void)hipEventDestroy(ev->polled);
    delete ev;
  });
}

int32_t qlx_evaluator_run(qlx_evaluator* ev, qlx_model* m, qlx_eval_summary* out) {
  return guard([&] {
    QLX_CHECK(ev && m && out, QLX_E_INVALID, "null argument");
    QLX_CHECK(m->device == ev->device, QLX_E_INVALID, "model and evaluator are on different devices");
    evaluator_run(ev, m, SelectBuiltin{}, out);
  });
}

int32_t qlx_evaluator_run_head(qlx_evaluator* ev, qlx_head* h, const qlx_dist* dist, qlx_eval_summary* out) {
  return guard([&] {
    QLX_CHECK(ev, QLX_E_INVALID, "null evaluator");
    QLX_CHECK(h, QLX_E_INVALID, "null head");
    dist_check(dist);
    QLX_CHECK(out, QLX_E_INVALID, "null out");
    const qlx_dist d = *dist;
    QLX_CHECK((int64_t)3 * d.atoms == (int64_t)h->width, QLX_E_INVALID, "3 * dist->atoms is not the head's width");
    QLX_CHECK(h->model->device == ev->device, QLX_E_INVALID, "model and evaluator are on different devices");
    evaluator_run(ev, h->model, SelectHead{h, d}, out);
  });
}

int32_t qlx_evaluator_episodes(qlx_evaluator* ev, float* returns, uint32_t* lengths, uint8_t* terminals, float* max_q_sums) {
  return guard([&] {
    QLX_CHECK(ev, QLX_E_INVALID, "null evaluator");
    QLX_CHECK(ev->has_run, QLX_E_STATE, "no evaluation has run");
    if (returns) std::copy(ev->rec_ret.begin(), ev->rec_ret.end(), returns);
    if (lengths) std::copy(ev->rec_len.begin(), ev->rec_len.end(), lengths);
    if (terminals) std::copy(ev->rec_term.begin(), ev->rec_term.end(), terminals);
    if (max_q_sums) std::copy(ev->rec_qsum.begin(), ev->rec_qsum.end(), max_q_sums);
  });
}

qlx_env* qlx_evaluator_env(qlx_evaluator* ev) { return ev ? ev->env : nullptr; }

}  // extern "C"
