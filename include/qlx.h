/* qlx.h — C ABI of the MI355X-native DQN hot path (env-step -> replay-sample -> Q-net update).
 *
 * This is the drop-in boundary for bitmagier/q-learning's Breakout DQN path.  Every entry point
 * names the reference interface it replaces (paths relative to the reference repo root):
 *
 *   ql::Environment / ql::Action         src/ql/src/prelude.rs:12-63
 *   BreakoutEnvironment (+ mechanics)   src/_breakout-ml/src/breakout_environment.rs:131-207,
 *                                        src/breakout-game/src/mechanics.rs:56-135
 *   ReplayBuffer / get_many             src/ql-with-tensorflow/src/learn/replay_buffer.rs:52-138
 *   generate_distinct_random_ids        src/ql-with-tensorflow/src/learn/self_driving_tf_q_learner.rs:276-296
 *   DeepQLearningModel                  src/ql-with-tensorflow/src/ml_model/model.rs:29-77
 *   SelfDrivingQLearner / Parameter     src/ql-with-tensorflow/src/learn/self_driving_tf_q_learner.rs:20-139
 *   BallGameTestEnvironment (2nd env)   src/ql/src/test/ballgame_test_environment.rs:12-262,
 *                                        src/ql-with-tensorflow/src/test/ballgame_test_env_addons.rs:7-50,
 *                                        src/ql-with-tensorflow/python_model/create_ql_model_ballgame_3x3x4_5_512.py
 *
 * Conventions
 *   - Opaque handles; every call returns int32_t status (QLX_OK = 0, < 0 = error) and
 *     qlx_last_error() returns a thread-local message.  This replaces the reference's
 *     panic!/anyhow::Result (q_learning_model.rs:125,147; mechanics.rs:265,284,303,511).
 *   - Host pointers are caller-owned.  Functions with a `_dev` suffix take device pointers and
 *     enqueue on the object's HIP stream without synchronising (chain them; qlx_*_sync to wait).
 *   - Calls on one handle are externally synchronised (the reference is single-threaded: Rc +
 *     ThreadRng are !Send).
 *   - Observation layout exposed to callers is the reference tensor view [n][x][y][slot] u8
 *     (breakout_environment.rs:44-50: H axis = x, channel = ring slot, raw 0..255).
 *   - No PyTorch/TF types; plain pointers and sizes only.
 */
#ifndef QLX_H
#define QLX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QLX_OK 0
#define QLX_E_INVALID (-1)
#define QLX_E_HIP (-2)
#define QLX_E_OOM (-3)
#define QLX_E_STATE (-4)
#define QLX_E_COMM (-5)
#define QLX_E_IO (-6)

#define QLX_ENV_BREAKOUT 1
#define QLX_ENV_BALLGAME 2
/* Conv(32,8,s4)-Conv(64,4,s2)-Conv(64,3,s1)-Dense512-Dense3 in fp32: the reference's arithmetic, every reduction a
 * single fmaf chain in the order DESIGN.md §6 defines (bit-exact against the CPU oracle) */
#define QLX_ARCH_NATURE_DQN 1
/* the same net with bf16 MFMA operands, fp32 accumulation and fp32 master weights (the labelled fast path) */
#define QLX_ARCH_NATURE_DQN_BF16 2
/* fp32 weight gradients of the conv layers: per-chunk fmaf chains over this many samples, chunks summed in order */
#define QLX_F32_WGRAD_CHUNK_CONV1 2   /* round 6: 4 -> 2 (twice the conv1 weight-gradient blocks: 36.2 -> 31.1 us at B = 1024); the oracle follows it */
#define QLX_F32_WGRAD_CHUNK_CONV2 16
#define QLX_F32_WGRAD_CHUNK_CONV3 16

const char* qlx_last_error(void);
int32_t qlx_version(void);

/* ---------------- Environment (ql::Environment for Breakout, batched) ---------------- */

/* Mechanics snapshot of one env, for parity checks (BreakoutMechanics, mechanics.rs:46-54). */
typedef struct qlx_breakout_state {
  float ball_x, ball_y, dir_x, dir_y;
  float panel_min_x, panel_min_y, panel_max_x, panel_max_y, panel_speed;
  uint32_t score, finished, next_slot, fault, reset_count;
  uint64_t bricks; /* bit i = brick i (creation order) still present */
} qlx_breakout_state;

typedef struct qlx_env qlx_env;

/* Action::ACTION_SPACE (breakout_environment.rs:103; BallGame 5, ballgame_test_environment.rs:239) */
int32_t qlx_env_action_space(int32_t kind);
/* Environment::episode_reward_goal_mean (breakout_environment.rs:203-206): bricks - 1 = 59; BallGame 9.5 (:88) */
float qlx_env_reward_goal_mean(int32_t kind);

/* BreakoutEnvironment::new x n_envs on `device`; env i draws its ball launch angle from the
 * build's counter-based stream (seed, i, reset_count) instead of thread_rng (mechanics.rs:103). */
int32_t qlx_env_create(int32_t kind, uint32_t n_envs, uint64_t seed, int32_t device, qlx_env** out);
int32_t qlx_env_destroy(qlx_env* env);
uint32_t qlx_env_count(const qlx_env* env);
/* Environment::reset (breakout_environment.rs:177-180) for every env, or where mask[i] != 0. */
int32_t qlx_env_reset(qlx_env* env, const uint8_t* mask_or_null);
/* Environment::step (breakout_environment.rs:184-201) for all envs; host arrays of n_envs.
 * Invalid actions (>= 3) fail with QLX_E_INVALID like Action::try_from_numeric. */
int32_t qlx_env_step(qlx_env* env, const uint8_t* actions, float* rewards, uint8_t* dones);
/* Device-pointer form: actions/rewards/dones are device arrays of n_envs. */
int32_t qlx_env_step_dev(qlx_env* env, const uint8_t* d_actions, float* d_rewards, uint8_t* d_dones);
/* ToMultiDimArray::batch_to_multi_dim_array view of the current states: out[n][84][84][4] (x,y,slot). */
int32_t qlx_env_obs(qlx_env* env, uint8_t* out);
int32_t qlx_env_states(qlx_env* env, qlx_breakout_state* out /* [n_envs] */);
/* Directed start states (the mirror of qlx_bg_env_set_states): copies in[n_envs] over the mechanics on the env's
 * stream and zeroes the per-episode step counts.  The ring frames, the running checksums and the sticky flags stay
 * as they are.  QLX_E_INVALID, with nothing written, if any state has finished > 1, next_slot > 3 or
 * bricks >= 2^60.  Floats are taken as given, NaN and infinity included: every loop of the physics tick is bounded
 * (at most 65 moves per tick and 65 probes per bisection, either exhaustion raising fault bit 4), so no state can
 * hang a step. */
int32_t qlx_env_set_states(qlx_env* env, const qlx_breakout_state* in /* [n_envs] */);
/* Steps taken by each env in its current episode (what the learner compares with max_steps_per_episode). */
int32_t qlx_env_episode_steps(qlx_env* env, uint32_t* out /* [n_envs] */);
/* Running per-env checksum of every step (state + new frame), see DESIGN.md §parity. */
int32_t qlx_env_hashes(qlx_env* env, uint64_t* out /* [n_envs] */);
int32_t qlx_env_sync(qlx_env* env);

/* ---------------- Replay buffer (ReplayBuffer, HBM-resident) ---------------- */

typedef struct qlx_replay qlx_replay;

/* FIFO of `capacity` transitions (history_buffer_len); logical index 0 = oldest (VecDeque). Frames
 * are stored once (s' of step t is s of step t+1), 7,056 B per transition + metadata. */
int32_t qlx_replay_create(uint64_t capacity, uint32_t n_envs, int32_t device, qlx_replay** out);
int32_t qlx_replay_destroy(qlx_replay* rb);
uint64_t qlx_replay_len(const qlx_replay* rb);
/* ReplayBuffer::add for the transition each env of `env` just made (actions = device array used for
 * that step, rewards/dones = its outputs).  Call once after every qlx_env_step[_dev]. */
int32_t qlx_replay_push_dev(qlx_replay* rb, qlx_env* env, const uint8_t* d_actions, const float* d_rewards,
                            const uint8_t* d_dones);
/* Host-array form of qlx_replay_push_dev (synchronises). */
int32_t qlx_replay_push(qlx_replay* rb, qlx_env* env, const uint8_t* actions, const float* rewards,
                        const uint8_t* dones);
/* generate_distinct_random_ids::<B>(rng, 0..len) from stream (seed, update_idx, rank); host out[B]. */
int32_t qlx_replay_sample_distinct(qlx_replay* rb, uint64_t seed, uint32_t update_idx, uint32_t rank, uint32_t batch,
                                   uint64_t* out_indices);
/* ReplayBuffer::get_many + batch_to_multi_dim_array: host outputs, any may be NULL. */
int32_t qlx_replay_get_many(qlx_replay* rb, const uint64_t* indices, uint32_t batch, uint8_t* s /*[B][84][84][4]*/,
                            uint8_t* s_next, uint8_t* actions, float* rewards, uint8_t* dones);
/* n-step return windows (beyond the reference; DESIGN.md §6 "n-step returns").  The window of the transition at a
 * logical index runs over the same env's following transitions (n_envs push positions apart) and ends after n_step
 * of them, at a done, at the newest pushed transition, or where the episode ended without a done (the next slot's
 * episode step is not this one's + 1).  Per index: returns = sum_{j<m} gamma^j r_j, discounts = gamma^m (fp32, one
 * rounding per multiply and per add), last_indices = logical index of the window's last transition, terminals = its
 * done, steps = m.  Host outputs, any may be NULL; synchronises.  n_step 1 gives (reward, gamma, index, done, 1).
 * QLX_E_INVALID for n_step 0, n_step > QLX_NSTEP_MAX or an index >= len. */
#define QLX_NSTEP_MAX 32
int32_t qlx_replay_nstep(qlx_replay* rb, const uint64_t* indices, uint32_t batch, uint32_t n_step, float gamma,
                         float* returns, float* discounts, uint64_t* last_indices, uint8_t* terminals, uint32_t* steps);

/* ---------------- Q-network (DeepQLearningModel) ---------------- */

typedef struct qlx_model qlx_model;

/* Nature-DQN (arch QLX_ARCH_NATURE_DQN = fp32, QLX_ARCH_NATURE_DQN_BF16 = bf16 MFMA operands) with GlorotUniform
 * weights from stream (seed, var, 0) and zero biases; fp32 master weights + Adam slots in HBM.  lr 2.5e-4, beta
 * 0.9/0.999, eps 1e-7, clipnorm 1. */
int32_t qlx_model_create(int32_t arch, uint64_t seed, int32_t device, qlx_model** out);
int32_t qlx_model_destroy(qlx_model* m);
int32_t qlx_model_num_vars(void);
/* The optimizer hyperparameters every model is created with, out[5] = {learning_rate, beta_1, beta_2, epsilon, clipnorm}
 * (float32; the reference's Keras optimizer_config, keras_metadata.pb; no device needed). */
int32_t qlx_model_hparams(float* out);
int64_t qlx_model_var_size(int32_t var);
/* which: 0 = weights, 1 = Adam m, 2 = Adam v.  Layout = Keras HWIO / [in,out]. */
int32_t qlx_model_get_var(qlx_model* m, int32_t var, int32_t which, float* out);
int32_t qlx_model_set_var(qlx_model* m, int32_t var, int32_t which, const float* in);
int64_t qlx_model_iterations(qlx_model* m);
int32_t qlx_model_copy_weights(qlx_model* dst, const qlx_model* src);
/* predict_action for n states (model.rs:39-42): q_out [n][3] (may be NULL), actions [n] = argmax. */
int32_t qlx_model_predict(qlx_model* m, const uint8_t* obs /*[n][84][84][4]*/, uint32_t n, float* q_out,
                          uint8_t* actions);
/* batch_predict_max_future_reward (model.rs:44-47). */
int32_t qlx_model_batch_max_q(qlx_model* m, const uint8_t* obs, uint32_t n, float* out);
/* train (model.rs:49-65): forward, Huber(1) mean, backward, clip_by_norm(1) per variable, Adam.
 * loss_out (may be NULL) gets the batch loss; grads_out (may be NULL) the raw gradients of all vars
 * concatenated; norms_out (may be NULL) the 10 per-variable L2 norms before clipping. */
int32_t qlx_model_train(qlx_model* m, const uint8_t* obs, const uint8_t* actions, const float* y, uint32_t batch,
                        float* loss_out, float* grads_out, float* norms_out);
// Test hook of the data-parallel update tail (round 6): clip_by_norm(grads * scale) per variable + legacy Adam
// (ResourceApplyAdam, iterations + 1) on host gradients [1,685,667] in the flat variable order, as learner_update runs the
// tail after an all-reduce with scale = 1 / world (self_driving_tf_q_learner.rs:201 train -> q_learning_model.rs:165-189,
// split by the build's DP).  norms_out [10] (or NULL): the clip norms of the scaled gradient.
int32_t qlx_model_apply_gradient(qlx_model* m, const float* grads, float scale, float* norms_out);
/* Load a TF SavedModel / checkpoint bundle of the reference Breakout model (layer_with_weights-0..4 kernel /
 * bias, OPTIMIZER_SLOT m / v, optimizer/iter; shapes checked against saved/ql_model_breakout_84x84x4_3_32). */
int32_t qlx_model_load_tf(qlx_model* m, const char* bundle_prefix);
/* Debug view of intermediate activations of the last predict: layer 1..4 as fp32 host arrays. */
int32_t qlx_model_last_activation(qlx_model* m, int32_t layer, float* out);
/* write_checkpoint (model.rs:67-70): weights + Adam slots + iterations in a flat file. */
int32_t qlx_model_write_checkpoint(qlx_model* m, const char* path);
int32_t qlx_model_read_checkpoint(qlx_model* m, const char* path);
int32_t qlx_model_sync(qlx_model* m);

/* ---------------- Learner (SelfDrivingQLearner) ---------------- */

typedef struct qlx_params { /* Parameter (self_driving_tf_q_learner.rs:20-67) + build fields */
  float gamma;
  float lowest_episode_reward_goal_threshold_pct;
  double epsilon_max;
  double epsilon_min;
  double epsilon_greedy_steps;
  uint64_t max_steps_per_episode;
  uint64_t epsilon_pure_random_steps;
  uint64_t history_buffer_len;
  uint64_t update_after_actions;
  uint64_t target_sync_steps; /* 0 = never (reference behaviour) */
  uint64_t episode_reward_history_buffer_len;
  uint32_t n_envs;
  uint32_t batch_size;
  uint64_t env_seed;
  uint64_t learner_seed;
  uint64_t init_seed;
  uint32_t rank;
  uint32_t flags;     /* QLX_LEARNER_* extensions beyond the reference (0 = the reference algorithm) */
  float per_alpha;    /* prioritized replay: P(i) ~ p_i^alpha, p_i = |td_i| + per_eps */
  float per_beta;     /* importance-sampling exponent, w_i = (len P(i))^-beta / max_batch w */
  float per_eps;
  uint32_t qnet_precision;     /* QLX_PREC_F32 (0, the reference's arithmetic) or QLX_PREC_BF16 */
  uint64_t stats_after_steps;  /* every this many env-steps: checkpoint + learning_update_log (0 = never) */
  char checkpoint_file[256];   /* write_checkpoint target of those events and of solved() (empty = not written) */
  float episode_reward_goal;   /* goal solved() tests (Environment::episode_reward_goal_mean, prelude.rs); NaN (the
                                  qlx_params_default value) = the env's own (Breakout: bricks - 1,
                                  breakout_environment.rs:203-206); any other value, 0 included, mocks it.
                                  ABI semantics change in round 4: 0 used to select the env's goal; a zero-filled
                                  struct now mocks a goal of 0 (qlx_learner_create warns on stderr) */
  uint32_t n_step;             /* n-step returns (beyond the reference): y = sum_{j<m} gamma^j r_{t+j} + gamma^m max_a
                                  Q_target(s_{t+m}), m <= n_step (qlx_replay_nstep's window).  0 and 1 (zero-filled and
                                  qlx_params_default structs read 0) = the reference's 1-step target, unchanged;
                                  2..QLX_NSTEP_MAX = n-step; larger values fail in qlx_learner_create.  Breakout learner
                                  only: qlx_bg_learner_create fails with n_step > 1.  The field fills what was tail
                                  padding: sizeof(qlx_params) stays 408 */
} qlx_params;
#ifdef __cplusplus
static_assert(sizeof(qlx_params) == 408, "qlx_params ABI size");
#endif

#define QLX_PREC_F32 0u
#define QLX_PREC_BF16 1u

/* qlx_params.flags */
#define QLX_LEARNER_DOUBLE_DQN 1u  /* y = r + gamma Q_target(s', argmax_a Q_online(s')) (van Hasselt et al. 2016) */
#define QLX_LEARNER_PER 2u         /* proportional prioritized replay on an HBM sum tree (Schaul et al. 2016) */

void qlx_params_default(qlx_params* p);

typedef struct qlx_learner qlx_learner;

typedef struct qlx_learner_stats {
  uint64_t step_count, vec_steps, update_count, episode_count, replay_len, solved;
  double epsilon;
  float running_reward, last_loss;
} qlx_learner_stats;

/* SelfDrivingQLearner::new: owns a batched env, replay, online + target ("stabilized") model. */
int32_t qlx_learner_create(const qlx_params* p, int32_t device, qlx_learner** out);
int32_t qlx_learner_destroy(qlx_learner* l);
/* One vector step (n_envs env-steps + the updates they trigger), enqueued asynchronously. */
int32_t qlx_learner_vector_step(qlx_learner* l);
int32_t qlx_learner_run(qlx_learner* l, uint64_t n_vector_steps);
/* Vector steps without updates (act, env step, replay push, episode books; epsilon and step_count advance): fills the
 * replay before a measurement or a parity check at a given replay occupancy.  Not in the reference loop. */
int32_t qlx_learner_prefill(qlx_learner* l, uint64_t n_vector_steps);
/* End the current episode of every env with mask[e] != 0 now, as reaching max_steps_per_episode does (learn_episode
 * :214-224: the episode's reward enters the reward history, episode_count advances, the env resets); no transition is
 * added.  mask: host array [n_envs].  Lets a measurement start the envs' episodes at staggered steps (all envs launch
 * together, so with a short-lived policy their episodes otherwise end in waves).  Not in the reference loop.  Data
 * parallel: a collective (the global solved() statistics are all-reduced), so every rank calls it. */
int32_t qlx_learner_end_episodes(qlx_learner* l, const uint8_t* mask);
/* learn_till_mastered (self_driving_tf_q_learner.rs:127-132): vector steps until solved() or max_vector_steps. */
int32_t qlx_learner_learn_till_mastered(qlx_learner* l, uint64_t max_vector_steps, uint64_t* steps_run);
/* Statistics events so far (write_checkpoint + learning_update_log every stats_after_steps env-steps and on solved,
 * :204-212,226-230); the last event's log text; a callback receiving each log text (the reference's log::info!). */
uint64_t qlx_learner_stats_events(const qlx_learner* l);
int32_t qlx_learner_last_log(qlx_learner* l, char* buf, size_t cap, size_t* len);
int32_t qlx_learner_set_log_callback(qlx_learner* l, void (*cb)(const char* text, void* user), void* user);
int32_t qlx_learner_sync(qlx_learner* l);
int32_t qlx_learner_stats_get(qlx_learner* l, qlx_learner_stats* out);
/* Outputs of the last vector step (host copies; synchronises): actions/rewards/dones [n_envs],
 * losses [n_updates], indices [n_updates][B], targets [n_updates][B] (with n_step > 1 the n-step y); any may be
 * NULL. Returns the number of updates of that step in *n_updates. */
int32_t qlx_learner_last(qlx_learner* l, uint8_t* actions, float* rewards, uint8_t* dones, float* losses,
                         uint64_t* indices, float* targets, uint32_t* n_updates);
/* Prioritized replay state (learner created with QLX_LEARNER_PER): IS weights of the last vector step's batches
 * [n_updates][B], the sum tree's leaves [history_buffer_len] (priority^alpha per physical replay slot), the
 * priority new transitions enter with; any may be NULL. */
int32_t qlx_learner_priorities(qlx_learner* l, float* is_weights, float* leaves, float* per_max);
/* Frame sparsity of the last vector step (diagnostic, not on the hot path; synchronises): the fractions of the fp32
 * conv work the exact zero skips leave out, in the kernels' own units - out[0..3] over the step's sampled training
 * states (NaN when the step ran no update), out[4..7] over the current acting frames (the observations the next
 * vector step acts on: after this step's env step and resets), each {conv1 forward all-zero steps,
 * conv1 weight-gradient all-zero steps, conv2 background rows, conv3 background rows}. */
int32_t qlx_learner_frame_sparsity(qlx_learner* l, double* out);
/* Learning statistics (learning_update_log, self_driving_tf_q_learner.rs:235-273): per-action counts over the
 * replay's actions [3] (device histogram), the episode reward history oldest first (n = entries, up to cap
 * copied), and the log text itself (UTF-8; *len = full length, buf gets up to cap - 1 bytes + NUL).  Actions are
 * listed in numeric order (the reference iterates a hash map). */
int32_t qlx_learner_action_counts(qlx_learner* l, uint64_t* counts);
int32_t qlx_learner_episode_rewards(qlx_learner* l, float* out, uint64_t cap, uint64_t* n);
int32_t qlx_learner_update_log(qlx_learner* l, char* buf, size_t cap, size_t* len);
qlx_env* qlx_learner_env(qlx_learner* l);
qlx_replay* qlx_learner_replay(qlx_learner* l);
qlx_model* qlx_learner_model(qlx_learner* l, int32_t which /* 0 online, 1 target */);
/* Data-parallel: RCCL communicator over world ranks (one process per GPU); gradients are
 * all-reduced (mean) before clip_by_norm + Adam. uid from qlx_dist_unique_id on rank 0. */
int32_t qlx_dist_unique_id(uint8_t out[128]);
int32_t qlx_learner_dist_init(qlx_learner* l, int32_t world, int32_t rank, const uint8_t uid[128]);
/* Rank count of the learner's RCCL communicator as RCCL reports it (ncclCommCount); 1 without dist_init.  At world W
 * every update averages W per-rank batches of batch_size samples: the global batch per update is W x batch_size. */
int32_t qlx_learner_comm_size(qlx_learner* l, int32_t* world);
/* Kernel timing with HIP events on the learner stream.  Scopes are named per kernel ("conv1_fwd",
 * "conv1_wgrad", "fc1_fwd", "adam", "env_step", "replay_push", ...) or per phase ("act_forward",
 * "gather", "sample"); each carries its algorithmic work (FLOPs for GEMM kernels, bytes for
 * HBM-bound ones).  filter = one scope name records only that scope (NULL = all). */
int32_t qlx_learner_profile(qlx_learner* l, int32_t enable);
int32_t qlx_learner_profile_filter(qlx_learner* l, const char* name_or_null);
/* filter + sampling: record every stride-th launch of that scope (dispatch-bound events, see profiler.h) */
int32_t qlx_learner_profile_sample(qlx_learner* l, const char* name_or_null, uint32_t stride);
int32_t qlx_learner_profile_get(qlx_learner* l, const char* name, double* total_us, double* total_work,
                                uint64_t* launches);
int32_t qlx_learner_profile_names(qlx_learner* l, char* buf, size_t cap);

/* ---------------- Policy evaluation (beyond the reference) ----------------
 * n_envs fresh Breakout envs play episodes_per_env episodes each with a model's current weights, greedily or at a
 * fixed epsilon, entirely on the GPU; nearest reference interfaces: render_ballgame_cases.rs (a trained model replayed
 * over initial states) and learn_episode's acting branch (self_driving_tf_q_learner.rs:153-167).  Per vector step
 * t = 0, 1, ... and env e still playing: q = Q(obs_e); the action is random (uniform over 3, word 2 of stream
 * (policy_seed, e, t, purpose 8)) when epsilon > 0 and epsilon > the f64 from words 0-1 of that stream, else the first
 * argmax of q; return and max_a q accumulate in fp32 in step order; an episode ends at done or after
 * max_steps_per_episode steps, is recorded, and the env resets; an env retires after its last episode (it is still
 * stepped with action 0, nothing of it is counted).  The Q-net forward runs over the envs still playing only, as
 * counted at the last poll (DESIGN.md "Policy evaluation"). */
#define QLX_EVAL_MAX_ENVS 8192            /* one forward chunk (kF32FwdChunk) */
typedef struct qlx_eval_config {
  uint32_t n_envs;                  /* 1..QLX_EVAL_MAX_ENVS */
  uint32_t episodes_per_env;        /* K >= 1; n_envs * K <= 1<<24 */
  uint64_t max_steps_per_episode;   /* >= 1; an episode ends without done at this many steps, as in the learner */
  double   epsilon;                 /* finite, 0..1; 0 = greedy */
  uint64_t env_seed;                /* ball launch stream, env ids 0..n_envs-1, reset_count from 0 each run */
  uint64_t policy_seed;             /* epsilon draws */
  uint32_t poll_steps;              /* host reads the active count every this many vector steps; 0 = the default */
  uint32_t flags;                   /* must be 0 */
} qlx_eval_config;

typedef struct qlx_eval_summary {
  uint64_t episodes, env_steps, vector_steps, forward_samples, terminal_episodes;
  uint64_t action_counts[3];
  double   mean_return, mean_length, mean_max_q;   /* mean_max_q = sum of max_a q over all counted steps / env_steps */
  float    min_return, max_return;
} qlx_eval_summary;
#ifdef __cplusplus
static_assert(sizeof(qlx_eval_config) == 48, "qlx_eval_config ABI size");
static_assert(sizeof(qlx_eval_summary) == 96, "qlx_eval_summary ABI size");
#endif

typedef struct qlx_evaluator qlx_evaluator;
/* Argument errors (QLX_E_INVALID, the field named in qlx_last_error) are reported before the device is touched. */
int32_t qlx_evaluator_create(const qlx_eval_config* cfg, int32_t device, qlx_evaluator** out);
int32_t qlx_evaluator_destroy(qlx_evaluator* ev);
/* plays K episodes per env with m's current weights (either arch) on m's stream; m is not modified; synchronises.
 * Every run starts from the same env and draw state: equal config and weights give equal results.  vector_steps = the
 * first multiple of poll_steps at which no env was playing; forward_samples = the rows the Q-net forward ran over. */
int32_t qlx_evaluator_run(qlx_evaluator* ev, qlx_model* m, qlx_eval_summary* out);
/* (the policy of a distributional wide head: qlx_evaluator_run_head, with the head's calls below) */
/* records of the last run (of either kind), [n_envs][K] env-major, any may be NULL: return, length, ended by done, sum of max_a q */
int32_t qlx_evaluator_episodes(qlx_evaluator* ev, float* returns, uint32_t* lengths, uint8_t* terminals, float* max_q_sums);
qlx_env* qlx_evaluator_env(qlx_evaluator* ev);
/* evaluates the learner's online model on the learner's stream with a temporary evaluator; the learner's own
 * env, replay, counters, RNG positions, memo and profiler scopes are untouched.  Local to the rank (no collective). */
int32_t qlx_learner_evaluate(qlx_learner* l, const qlx_eval_config* cfg, qlx_eval_summary* out);

/* ---------------- Snapshots (beyond the reference) ----------------
 * A learner (or a replay alone) saved to one file and created again from it, so that a run continues bit for bit like one
 * that never stopped: every random draw here is a function of counters, and the file holds those counters with the env,
 * replay, both models, the episode books, the prioritized-replay leaves and the target memo (DESIGN.md "Snapshots").
 * Frames cross PCIe and reach the file packed on the GPU (QLX_FRAME_CODEC_BITMAP: a bitmap of the non-zero bytes and
 * those bytes, lossless); QLX_SNAPSHOT_PACK=0, read at save, stores them raw; a load accepts both.
 * Errors: arguments QLX_E_INVALID; anything wrong with a file (missing, short, bad magic, version, kind, a section past
 * the end, a checksum or the codec's own consistency) QLX_E_IO with a message naming it; a failed load creates nothing.
 * A save writes path + ".tmp" and renames it over path; two saves of equal state are byte-identical.  Not saved: the
 * profiler, the log callback, the RCCL communicator (a snapshot is local to its rank; qlx_learner_dist_init may follow
 * a load) and the last step's outputs (qlx_learner_last reports 0 updates until the next vector step). */
#define QLX_SNAPSHOT_VERSION 1
#define QLX_SNAPSHOT_LEARNER 1
#define QLX_SNAPSHOT_REPLAY  2
#define QLX_FRAME_CODEC_RAW    0
#define QLX_FRAME_CODEC_BITMAP 1

typedef struct qlx_snapshot_info {
  uint32_t format_version, kind, frame_codec, reserved;
  uint64_t step_count, vec_steps, update_count, episode_count, replay_len, replay_total;
  uint64_t frames, frame_bytes_raw, frame_bytes_stored, file_bytes;
  qlx_params params;            /* kind LEARNER; zero for REPLAY except n_envs, history_buffer_len */
} qlx_snapshot_info;
#ifdef __cplusplus
static_assert(sizeof(qlx_snapshot_info) == 504, "qlx_snapshot_info ABI size");
#endif

int32_t qlx_snapshot_info_read(const char* path, qlx_snapshot_info* out);        /* host only, no device */
int32_t qlx_learner_save(qlx_learner* l, const char* path);                      /* synchronises; local to the rank */
int32_t qlx_learner_load(const char* path, int32_t device, qlx_learner** out);   /* creates the learner from the file */
int32_t qlx_replay_save(qlx_replay* rb, const char* path);
int32_t qlx_replay_load(const char* path, int32_t device, qlx_replay** out);
/* test hook of the frame codec: host frames [n][7056] -> device -> pack -> packed_out (host, cap bytes) -> device ->
 * unpack -> frames_out; *packed_bytes = the packed size (QLX_E_INVALID when cap is smaller).  codec as above. */
int32_t qlx_frame_codec_roundtrip(const uint8_t* frames, uint32_t n, int32_t codec, int32_t device,
                                  uint8_t* packed_out, uint64_t cap, uint64_t* packed_bytes, uint8_t* frames_out);

/* ---------------- DBSCAN over f32 (src/ql/src/util/dbscan.rs:209-341) ----------------
 * cluster_analysis(values, max_neighbor_distance, core_point_min_neighbors) with Distance = |a - b|, exact, in
 * O(n log n): labels[i] = cluster position (clusters ordered by lowest member index, as the reference returns
 * them) or -1 for noise.  _format renders the reference's Display ("Yx(B..C), ..., Yx(noise)", :91-133).
 * Values and max_neighbor_distance must be finite, max_neighbor_distance >= 0. */
int32_t qlx_dbscan_f32(const float* values, uint64_t n, float max_neighbor_distance, uint64_t core_point_min_neighbors,
                       int32_t* labels, uint64_t* n_clusters);
int32_t qlx_dbscan_f32_format(const float* values, uint64_t n, float max_neighbor_distance, uint64_t core_point_min_neighbors,
                              char* buf, size_t cap, size_t* len);

/* ---------------- prioritized-replay sum tree (beyond the reference) ----------------
 * The learner's HBM sum tree as a standalone object: leaves = priorities of `capacity` slots, proportional
 * sampling of n_updates batches of `batch` draws (draw b of update u: stream (seed, first_update + u, rank,
 * purpose 7, word b)), IS weights (len P(i))^-beta normalised per batch, and last-writer-wins priority
 * updates p = (|td| + eps)^alpha.  Oracle: oracle/learner_ref.h SumTree / per_sample. */
typedef struct qlx_sumtree qlx_sumtree;
int32_t qlx_sumtree_create(uint64_t capacity, int32_t device, qlx_sumtree** out);
int32_t qlx_sumtree_destroy(qlx_sumtree* t);
int32_t qlx_sumtree_set_leaves(qlx_sumtree* t, const float* leaves /* [capacity], finite >= 0 */);
int32_t qlx_sumtree_get(qlx_sumtree* t, float* leaves, float* total, float* per_max);
int32_t qlx_sumtree_sample(qlx_sumtree* t, uint64_t seed, uint32_t first_update, uint32_t n_updates, uint32_t rank, uint64_t len,
                           float beta, uint32_t batch, uint64_t* slots /* [n_updates][batch] */, float* weights);
int32_t qlx_sumtree_update(qlx_sumtree* t, const uint64_t* slots, const float* td_abs, uint32_t n, float alpha, float eps);

/* ---------------- BallGame (BallGameTestEnvironment + its 3x3x4 -> 5 Q-model) ----------------
 * The reference's second Environment / DeepQLearningModel pair, batched on the GPU.  Same conventions as
 * above; actions West 0, North 1, East 2, South 3, Nothing 4 (ballgame_test_environment.rs:240-249). */

typedef struct qlx_ballgame_state { /* BallGameState (:92-97) */
  uint8_t field[9];                  /* index x * 3 + y: 0 empty, 1 goal, 2 ball, 3 obstacle */
  uint8_t ball_x, ball_y, pad;
  uint32_t steps;
  uint32_t reset_count;
} qlx_ballgame_state;

typedef struct qlx_bg_env qlx_bg_env;
/* BallGameTestEnvironment::new x n_envs: env i's random_initial_state (:100-123) draws gen_range(0..3) from
 * the build's stream (seed, i, reset_count, purpose 6) instead of thread_rng. */
int32_t qlx_bg_env_create(uint32_t n_envs, uint64_t seed, int32_t device, qlx_bg_env** out);
int32_t qlx_bg_env_destroy(qlx_bg_env* env);
int32_t qlx_bg_env_reset(qlx_bg_env* env, const uint8_t* mask_or_null);
/* Environment::step (:69-86) for all envs (host arrays of n_envs; actions >= 5 fail with QLX_E_INVALID). */
int32_t qlx_bg_env_step(qlx_bg_env* env, const uint8_t* actions, float* rewards, uint8_t* dones);
/* to_multi_dim_array: out[n][3][3][4] u8 one-hot (x, y, channel = entry). */
int32_t qlx_bg_env_obs(qlx_bg_env* env, uint8_t* out);
int32_t qlx_bg_env_states(qlx_bg_env* env, qlx_ballgame_state* out);
int32_t qlx_bg_env_set_states(qlx_bg_env* env, const qlx_ballgame_state* in);

typedef struct qlx_bg_model qlx_bg_model;
/* Conv(32, 2x2 same)-Conv(32, 1x1)-Dense512-Dense5 in fp32; GlorotUniform from stream (seed, var, 1);
 * 8 variables k0 [2,2,4,32] b0 k1 [1,1,32,32] b1 k2 [288,512] b2 k3 [512,5] b3. */
int32_t qlx_bg_model_create(uint64_t seed, int32_t device, qlx_bg_model** out);
/* as qlx_model_hparams, for the BallGame model (create_ql_model_ballgame_3x3x4_5_512.py's Adam) */
int32_t qlx_bg_model_hparams(float* out);
int32_t qlx_bg_model_destroy(qlx_bg_model* m);
int64_t qlx_bg_model_var_size(int32_t var);
int32_t qlx_bg_model_get_var(qlx_bg_model* m, int32_t var, int32_t which, float* out);
int32_t qlx_bg_model_set_var(qlx_bg_model* m, int32_t var, int32_t which, const float* in);
int64_t qlx_bg_model_iterations(qlx_bg_model* m);
int32_t qlx_bg_model_predict(qlx_bg_model* m, const uint8_t* obs /*[n][3][3][4]*/, uint32_t n, float* q_out, uint8_t* actions);
int32_t qlx_bg_model_batch_max_q(qlx_bg_model* m, const uint8_t* obs, uint32_t n, float* out);
/* train_model (.py:71-85): MSE of q_a, backward, clip_by_norm(1) per variable, Adam. */
int32_t qlx_bg_model_train(qlx_bg_model* m, const uint8_t* obs, const uint8_t* actions, const float* y, uint32_t batch,
                           float* loss_out, float* grads_out, float* norms_out);

/* Load a TF SavedModel / checkpoint bundle of the reference model (variables/variables.index + .data, e.g.
 * python_model/saved/ql_model_ballgame_3x3x4_5_512/variables/variables): weights, Adam m / v and iterations. */
int32_t qlx_bg_model_load_tf(qlx_bg_model* m, const char* bundle_prefix);

typedef struct qlx_bg_learner qlx_bg_learner;
/* SelfDrivingQLearner over BallGame (same qlx_params and vector-step semantics as qlx_learner).  n-step returns are
 * the Breakout learner's (this learner keeps a replay of its own): n_step > 1 fails with QLX_E_INVALID. */
int32_t qlx_bg_learner_create(const qlx_params* p, int32_t device, qlx_bg_learner** out);
int32_t qlx_bg_learner_destroy(qlx_bg_learner* l);
int32_t qlx_bg_learner_run(qlx_bg_learner* l, uint64_t n_vector_steps);
int32_t qlx_bg_learner_sync(qlx_bg_learner* l);
int32_t qlx_bg_learner_stats_get(qlx_bg_learner* l, qlx_learner_stats* out);
int32_t qlx_bg_learner_last(qlx_bg_learner* l, uint8_t* actions, float* rewards, uint8_t* dones, float* losses,
                            uint64_t* indices, float* targets, uint32_t* n_updates);
/* prioritized replay state of a learner created with QLX_LEARNER_PER (as qlx_learner_priorities) */
int32_t qlx_bg_learner_priorities(qlx_bg_learner* l, float* is_weights, float* leaves, float* per_max);
/* learning_update_log for BallGame: counts [5] by numeric action, reward history, log text (qlx_learner_* above) */
int32_t qlx_bg_learner_action_counts(qlx_bg_learner* l, uint64_t* counts);
int32_t qlx_bg_learner_episode_rewards(qlx_bg_learner* l, float* out, uint64_t cap, uint64_t* n);
int32_t qlx_bg_learner_update_log(qlx_bg_learner* l, char* buf, size_t cap, size_t* len);
qlx_bg_env* qlx_bg_learner_env(qlx_bg_learner* l);
qlx_bg_model* qlx_bg_learner_model(qlx_bg_learner* l, int32_t which /* 0 online, 1 target */);

/* ---------------- Training metrics (beyond the reference; its nearest interface is learning_update_log) ----------------
 * Opt-in, per learner: once enabled, every training update appends one 256-byte row to a ring in device memory (one small
 * kernel after the update's Adam, nothing copied, no synchronisation), and the host drains the ring whenever it likes.
 * With metrics off (the default, and after a load: not part of a snapshot) no launch, allocation or result changes.
 * All statistics are over the update's batch; means are accumulated in double in a fixed order and rounded to float once,
 * and every field is bit-reproducible from run to run.  Rows are local to the rank (no collective). */
typedef struct qlx_update_metrics {
  uint64_t update;        /* update_count before this update (0-based, consecutive) */
  uint64_t step_count;    /* learner step_count when the update was enqueued */
  uint32_t batch, n_actions, n_vars;   /* B; 3 (Breakout) / 5 (BallGame); 10 / 8 */
  uint32_t n_clipped;     /* variables v < n_vars with grad_norm[v] > clipnorm */
  uint32_t n_linear;      /* samples with |td| > 1 (Huber's linear branch; counted for BallGame's MSE too) */
  uint32_t n_nonfinite;   /* samples whose q_a or y is not finite (the float statistics are then only reproducible) */
  float loss;             /* the update's loss, the same bits qlx_learner_last reports */
  float q_taken_mean, q_taken_min, q_taken_max;   /* q_a = Q(s)[action] as the training head wrote it */
  float q_max_mean;       /* mean of max_a Q(s) */
  float action_gap_mean;  /* mean of (largest - second largest of Q(s)); 0 for exact ties */
  float y_mean, y_min, y_max;          /* the targets */
  float td_abs_mean, td_abs_max;       /* td = |q_a - y|, one fp32 subtraction */
  float weight_mean;      /* mean importance-sampling weight (prioritized replay), else 1.0f */
  float grad_norm_global; /* (float)sqrt(sum_{v<n_vars} (double)grad_norm[v]^2), v ascending */
  uint32_t reserved;      /* 0 */
  uint32_t argmax_counts[8];   /* samples per first-argmax action of Q(s); entries >= n_actions are 0 */
  float grad_norm[16];         /* pre-clip L2 norm per variable of the gradient Adam used (data parallel: of the reduced,
                                  scaled one); entries >= n_vars are 0 */
  uint32_t td_hist[16];        /* |td| by binary exponent, see qlx_metrics_td_bin */
} qlx_update_metrics;
#ifdef __cplusplus
static_assert(sizeof(qlx_update_metrics) == 256, "qlx_update_metrics ABI size");
#endif

/* Host only: the td_hist bin of |td| as the kernel computes it (from the exponent bits): bin 0 holds |td| < 2^-11
 * (0 and denormals included), bin k = 1..14 holds 2^(k-12) <= |td| < 2^(k-11), bin 15 holds |td| >= 8, +inf and NaN. */
int32_t qlx_metrics_td_bin(float td_abs);
/* A ring of `capacity` rows (and its pinned staging buffer), replacing any earlier one; recorded and unread restart at 0
 * while `update` carries on from update_count.  0 = metrics off and the ring freed; above 1 << 20: QLX_E_INVALID.
 * Synchronises.  The row of the r-th recorded update lands in slot r % capacity. */
int32_t qlx_learner_metrics_enable(qlx_learner* l, uint32_t capacity);
/* Host counters, no synchronisation: the capacity, the updates recorded since enable, and the rows a read would return
 * now (unread ones not yet overwritten).  QLX_E_STATE with metrics off. */
int32_t qlx_learner_metrics_info(qlx_learner* l, uint32_t* capacity, uint64_t* recorded, uint64_t* unread);
/* Synchronises the learner stream; up to `cap` of the oldest unread rows that still exist into out, oldest first (the
 * rest stay unread); *n = rows written, *dropped = unread rows that were overwritten since the previous read.
 * QLX_E_STATE with metrics off. */
int32_t qlx_learner_metrics_read(qlx_learner* l, qlx_update_metrics* out, uint64_t cap, uint64_t* n, uint64_t* dropped);
int32_t qlx_bg_learner_metrics_enable(qlx_bg_learner* l, uint32_t capacity);
int32_t qlx_bg_learner_metrics_info(qlx_bg_learner* l, uint32_t* capacity, uint64_t* recorded, uint64_t* unread);
int32_t qlx_bg_learner_metrics_read(qlx_bg_learner* l, qlx_update_metrics* out, uint64_t cap, uint64_t* n, uint64_t* dropped);

/* ---------------- TF tensor bundles (the reference's model / checkpoint storage) ----------------
 * Host-only reader of variables.index (SSTable of BundleEntryProto) + variables.data-*; block and tensor
 * crc32c are verified.  Replaces SavedModelBundle::load's variable restore (q_learning_model.rs:47-52). */
typedef struct qlx_tf_bundle qlx_tf_bundle;
int32_t qlx_tf_bundle_open(const char* prefix /* ".../variables/variables" */, qlx_tf_bundle** out);
int32_t qlx_tf_bundle_close(qlx_tf_bundle* b);
int32_t qlx_tf_bundle_count(const qlx_tf_bundle* b);
/* dtype: TF DataType enum (1 = float, 9 = int64); dims: up to 8 */
int32_t qlx_tf_bundle_entry(const qlx_tf_bundle* b, int32_t i, char* name, size_t cap, int32_t* dtype, int64_t* dims,
                            int32_t* ndims, int64_t* nbytes);
int32_t qlx_tf_bundle_read(const qlx_tf_bundle* b, const char* name, void* out, size_t cap);

/* ---------------- Device-tensor env and replay calls (beyond the reference) ----------------
 * The env, the replay and its sampler for an agent that lives in device memory (a PyTorch module, say): every `_dev` call
 * below takes device pointers, enqueues on the object's stream and returns; none synchronises, allocates per call or
 * copies to the host (the replay reserves 32 KB of scratch and its flag word at the first such call and keeps them).
 * Argument errors (QLX_E_INVALID, the field named in qlx_last_error) are found on the host before anything is launched:
 * a null handle or out, an unknown layout, batch 0 or > 4096, n_step 0 or > QLX_NSTEP_MAX, a state pointer that is not
 * 16-byte aligned, batch > len for sampling.  An index >= len cannot be seen on the host: the kernels read nothing for it,
 * write an all-zero sample (states 0, actions 0, returns 0, discounts 0, terminals 1, last_indices = the index, steps 0)
 * and set a sticky flag in device memory that qlx_replay_sync reports as QLX_E_INVALID, once, and clears (the env's
 * bad-action flag pattern, qlx_env_sync).
 * State layouts, both u8 and dense, 28,224 bytes per state: */
#define QLX_OBS_NHWC_SLOT 0  /* [n][84][84][4] (x, y, ring slot): the bytes qlx_env_obs / qlx_replay_get_many give */
#define QLX_OBS_NCHW_TIME 1  /* [n][4][84][84] (age, x, y): channel 0 oldest ... 3 newest */
/* NCHW_TIME is read off the ring: the env's channel c is ring slot (next_slot + c) & 3; for a replay transition of
 * episode step k, channel c of s' is slot (k + c) & 3 and of s slot (k - 1 + c) & 3, that is the frame of episode step
 * k - 3 + c (s') or k - 4 + c (s), and zeros for steps below 1. */

/* the object's HIP stream (a hipStream_t) */
int32_t qlx_env_stream(qlx_env* env, void** hip_stream_out);
int32_t qlx_replay_stream(qlx_replay* rb, void** hip_stream_out);
/* the replay gives up its own stream (after waiting for it) and runs on the env's from now on, so that pushes, which run
 * on the env's stream, and batches are ordered without events; the env must outlive the replay.  Same device only. */
int32_t qlx_replay_share_stream(qlx_replay* rb, qlx_env* env);
/* waits for the replay's stream; QLX_E_INVALID once if a _dev call since the last sync met an index >= len */
int32_t qlx_replay_sync(qlx_replay* rb);

/* the current states of all envs in `layout` into d_out [n_envs] states */
int32_t qlx_env_obs_dev(qlx_env* env, int32_t layout, uint8_t* d_out);
/* qlx_env_reset with a device mask [n_envs] (or NULL: every env) */
int32_t qlx_env_reset_dev(qlx_env* env, const uint8_t* d_mask_or_null);

/* qlx_replay_sample_distinct into a device array [batch] */
int32_t qlx_replay_sample_distinct_dev(qlx_replay* rb, uint64_t seed, uint32_t update_idx, uint32_t rank, uint32_t batch,
                                       uint64_t* d_out_indices);

typedef struct qlx_batch_dev {     /* device pointers [batch], any may be NULL */
  uint8_t* s; uint8_t* s_next;     /* states in `layout`; s_next = s' of the n-step window's LAST transition */
  uint8_t* actions; float* returns; float* discounts; uint8_t* terminals;
  uint64_t* last_indices; uint32_t* steps;   /* qlx_replay_nstep's definitions, unchanged */
} qlx_batch_dev;
#ifdef __cplusplus
static_assert(sizeof(qlx_batch_dev) == 64, "qlx_batch_dev ABI size");
#endif
/* qlx_replay_get_many + qlx_replay_nstep for the logical indices in d_indices [batch] (device), on the replay's stream */
int32_t qlx_replay_batch_dev(qlx_replay* rb, const uint64_t* d_indices, uint32_t batch, uint32_t n_step, float gamma,
                             int32_t layout, const qlx_batch_dev* out);

/* ---------------- Q-network on device tensors (beyond the reference) ----------------
 * The Q-net's forward and its whole update (forward, Huber, backward, clip_by_norm, Adam) for an agent that computes its
 * own targets in device memory: states are read where they lie (dense device states, the replay ring through logical
 * indices, or an env's current ring), actions, targets, per-sample weights and all results are device arrays.  The
 * conventions are those of the section above: arguments are checked on the host, then everything is enqueued on the
 * model's stream; no `_dev` call synchronises, allocates or copies to the host.  qlx_model_reserve is the one call that
 * sizes the workspace: a `_dev` call with n above the reserved size (or before any reserve) fails with QLX_E_STATE and
 * launches nothing.  (The backward's gradient buffers are the backend's own and grow, once, at the first training batch
 * larger than any before, as they do for qlx_model_train and the learner.)
 * Host checks (QLX_E_INVALID, the field named in qlx_last_error), made before any handle is read: a null model, src or
 * required pointer; not exactly one state source; indices without replay or the reverse; an unknown layout; which not
 * 0 / 1; obs not 16-byte aligned; n 0 or > 8192; batch 0 or > 4096; all outputs of qlx_model_q_dev null.  After the
 * handle is read: the reserve check (QLX_E_STATE), an env or replay on another device, an env whose count is not n.
 * Data the host cannot see: an index >= len reads nothing and is the all-zero state; an action >= 3 trains as action 0
 * (the kernels read a checked copy); either sets a sticky flag that qlx_model_sync reports as QLX_E_INVALID, once. */
typedef struct qlx_states_dev {          /* exactly one source: obs, or replay + indices, or env */
  const uint8_t*  obs;       /* dense device states [n] in `layout`, 16-byte aligned */
  qlx_replay*     replay;    /* with indices: the transitions at these logical indices ... */
  const uint64_t* indices;   /* ... device array [n] */
  qlx_env*        env;       /* the env's current states; n must equal its env count */
  int32_t         layout;    /* QLX_OBS_NHWC_SLOT / QLX_OBS_NCHW_TIME: the channel order the net sees, for every source */
  int32_t         which;     /* replay source: 0 = s, 1 = s' of that transition (pass a batch's last_indices for n-step) */
} qlx_states_dev;
#ifdef __cplusplus
static_assert(sizeof(qlx_states_dev) == 40, "qlx_states_dev ABI size");
#endif
/* `layout` is the network's input-channel convention, not only the byte order of `obs`: NHWC_SLOT feeds ring slot j as
 * channel j (the reference's tensor view: what qlx_model_predict, qlx_model_train and the learner feed), NCHW_TIME feeds
 * the oldest frame as channel 0.  For the env and replay sources it only permutes the four frame pointers by the rules
 * above (env: slot (next_slot + c) & 3; replay: (k + c) & 3 for s', (k - 1 + c) & 3 for s; a frame the episode does not
 * have is a zero frame); no state byte moves.  Use a model with one convention throughout: the two train different nets. */

/* the model's HIP stream (a hipStream_t) */
int32_t qlx_model_stream(qlx_model* m, void** hip_stream_out);
/* the model gives up its own stream (after waiting for it) and runs on the env's from now on, as qlx_replay_share_stream;
 * the env must outlive the model.  Same device only. */
int32_t qlx_model_share_stream(qlx_model* m, qlx_env* env);
/* workspace for _dev calls of up to max_n states (1..8192), the flag word and the argument scratch; synchronises, may
 * allocate.  A smaller max_n than an earlier one changes nothing. */
int32_t qlx_model_reserve(qlx_model* m, uint32_t max_n);
/* Q(s) of n states: d_q [n][3], d_actions [n] = first argmax, d_max_q [n] = max_a Q; any may be NULL, not all three */
int32_t qlx_model_q_dev(qlx_model* m, const qlx_states_dev* src, uint32_t n, float* d_q, uint8_t* d_actions,
                        float* d_max_q);
/* one update as qlx_model_train runs it (forward, Huber(1) mean of weights * h, backward, clip_by_norm(1), Adam,
 * iterations + 1) on `batch` (1..4096) states with device actions [batch], targets d_y [batch] and optional per-sample
 * loss weights; d_loss (one float) and d_td_abs [batch] = |q_a - y| are optional outputs */
int32_t qlx_model_train_dev(qlx_model* m, const qlx_states_dev* src, const uint8_t* d_actions, const float* d_y,
                            const float* d_weights_or_null, uint32_t batch, float* d_loss_or_null, float* d_td_abs_or_null);
/* qlx_model_copy_weights without a host synchronisation: the copy runs on dst's stream behind what src's stream holds
 * now, and src's stream waits for it (nothing of either when they share a stream) */
int32_t qlx_model_copy_weights_dev(qlx_model* dst, qlx_model* src);
/* qlx_model_sync (above) also reports, once, a flag set by a _dev call since the last sync */

/* ---- a caller's own loss: backward and optimizer as separate steps ----
 * For a loss L(Q) computed outside the library the caller passes dq = dL/dQ [batch][3]; the backward gives the gradient of
 * sum_{b,n} dq[b][n] * Q(src)[b][n], i.e. dL/dvariables, through the same kernels as the built-in update (a dq row that is
 * zero except at the taken action reproduces that update's gradient value for value).  Same conventions and host checks as
 * above (a null model / src / d_dq / out pointer, the source's cases, batch 0 or > 4096, unknown step flags: QLX_E_INVALID
 * before any handle is read; then the reserve check QLX_E_STATE, device mismatches, the env count).
 * Source stability: the env and replay sources are read in place, by the forward and again by the backward (the conv1
 * weight gradient reads the frames).  The caller must not step the env or push into the replay between a forward and the
 * backward that belongs to it, and a dense `obs` passed to a recomputing backward must hold what the forward saw. */
#define QLX_STEP_GRADS_WRITTEN 1u  /* qlx_model_step_dev: the caller modified the buffer through qlx_model_grads_dev */
/* identifies the model's most recent forward pass (any caller); never 0 */
int32_t qlx_model_forward_ticket(qlx_model* m, uint64_t* ticket_out);
/* raw gradients of sum_{b,n} dq[b][n] * Q(src)[b][n] w.r.t. all ten variables -> the model's gradient buffer
 * (overwritten, not accumulated).  No clip, no Adam, iterations unchanged.  Enqueue only.  With `ticket` the model's
 * current ticket, that forward over `batch` samples and its activations still usable, no table is built and no forward
 * runs; otherwise, and always for ticket 0, the table is built from src and the trunk forward runs again.  Both ways give
 * identical gradients.  An index >= len behaves as in qlx_model_q_dev: zero state, sticky flag. */
int32_t qlx_model_backward_dev(qlx_model* m, const qlx_states_dev* src, const float* d_dq /*[batch][3]*/,
                               uint32_t batch, uint64_t ticket);
/* clip_by_norm per variable + Adam on the gradient buffer, iterations + 1.  QLX_E_STATE before any backward or train has
 * filled the buffer.  flags: 0 or QLX_STEP_GRADS_WRITTEN */
int32_t qlx_model_step_dev(qlx_model* m, uint32_t flags);
/* device pointer to the flat fp32 gradient buffer [1,685,667], variable order of qlx_model_train's grads_out;
 * valid for the model's lifetime */
int32_t qlx_model_grads_dev(qlx_model* m, float** d_grads_out, uint64_t* count_out);

/* ---- a wide output head: Z = a4 Wh + bh beside the model's own 512 -> 3 head ----
 * A dense layer 512 -> width (1..QLX_HEAD_MAX_WIDTH, any value) on a4, the ReLU output of fc1, attached to one fp32 model:
 * the outputs a dueling, categorical, quantile or bootstrapped agent needs from the same trunk, with forward, backward and
 * optimizer step, so its loss stays a few lines of the caller's own.  The head owns Wh [512][width] (GlorotUniform, fan_in
 * 512, fan_out width, from stream (seed, 10, 0, purpose 4) in element order) and bh [width] (zero), their Adam m and v, a
 * gradient buffer (Wh, then bh), its own iteration count and clip-norm scratch; it runs on the model's stream with the
 * model's hyperparameters (qlx_model_hparams).  The model's ten variables, its checkpoints, snapshots and learner do not
 * know the head: qlx_head_write_checkpoint / _read_checkpoint (below) are its persistence, weights, Adam slots and iterations;
 * qlx_head_get_var / _set_var move one array.
 * A model has at most one head (a second create: QLX_E_STATE); a bf16 model has none (QLX_E_INVALID); qlx_model_destroy of
 * a model with a live head fails with QLX_E_STATE.  Conventions of the `_dev` section above: arguments are checked on the
 * host before any handle is read (QLX_E_INVALID, the field named), then everything is enqueued on the model's stream; no
 * call but create, destroy and the host get / set synchronises, allocates or copies to the host; n is bounded by
 * qlx_model_reserve (QLX_E_STATE above it, nothing launched); an index >= len or a bad state source behaves as in
 * qlx_model_q_dev.  Arithmetic: every output is one fmaf chain in a fixed order, independent of the width,
 * of the column's position and of the batch; a width-3 head holding W4 and b4 gives the model's own Q, gradients and update
 * bit for bit. */
#define QLX_HEAD_MAX_WIDTH 1024
typedef struct qlx_head qlx_head;
int32_t qlx_head_create(qlx_model* m, uint32_t width, uint64_t seed, qlx_head** out);
int32_t qlx_head_destroy(qlx_head* h);
int32_t qlx_head_width(qlx_head* h);          /* -1 for a null head */
int64_t qlx_head_iterations(qlx_head* h);     /* -1 for a null head */
/* host arrays, synchronise: var 0 Wh [512][width], 1 bh [width]; which 0 weights, 1 Adam m, 2 Adam v */
int32_t qlx_head_get_var(qlx_head* h, int32_t var, int32_t which, float* out);
int32_t qlx_head_set_var(qlx_head* h, int32_t var, int32_t which, const float* in);
/* one trunk forward over n states (n <= the reserve), then both heads: d_z [n][width] and, unless NULL, d_q [n][3];
 * advances the model's forward ticket like any forward */
int32_t qlx_head_forward_dev(qlx_head* h, const qlx_states_dev* src, uint32_t n, float* d_z, float* d_q_or_null);
/* raw gradients of sum dz * Z + sum dq * Q (d_dz [batch][width]; d_dq [batch][3] or NULL: no Q term): the ten model
 * variables into the model's gradient buffer (W4 and b4 zero without dq), Wh and bh into the head's; both overwritten, not
 * accumulated.  batch 1..4096; the ticket rules are qlx_model_backward_dev's. */
int32_t qlx_head_backward_dev(qlx_head* h, const qlx_states_dev* src, const float* d_dz, const float* d_dq_or_null,
                              uint32_t batch, uint64_t ticket);
/* device pointer to the head's flat fp32 gradient buffer: Wh [512][width], then bh [width]; count = 513 * width */
int32_t qlx_head_grads_dev(qlx_head* h, float** d_grads_out, uint64_t* count_out);
/* qlx_model_step_dev steps the head as well (per-variable clip_by_norm and Adam, Wh and bh two variables with norms of
 * their own, the head's iterations + 1) when the gradient in the buffers came from qlx_head_backward_dev; after any other
 * backward, or a train call, it leaves the head alone. */
/* weights only, between heads of equal width on one device; orders the streams as qlx_model_copy_weights_dev does */
int32_t qlx_head_copy_weights_dev(qlx_head* dst, qlx_head* src);

/* ---- distributional losses on the wide head: QR-DQN's quantile Huber loss, C51's projected cross-entropy ----
 * A head of width 3 N read as Z[b][a N + i], action a in 0..2, atom i in 0..N-1 (z.view(-1, 3, N)).  The descriptor names
 * the reading; 3 * atoms must be the head's width (otherwise QLX_E_INVALID naming atoms, after the argument checks).
 * Values Q[b][a]: quantile - the mean of the N quantiles; categorical - sum_k p_k z_k, p = softmax(Z[b][a][:]) with the row
 * maximum subtracted, z_k = v_min + k D, D = (v_max - v_min) / (N - 1).  actions = first argmax, max_q its value.
 * Loss of a batch (live = terminals ? 0 : discounts; a* = a_star, or the first argmax of the values of z_next):
 *   quantile     T_j = returns + live z_next[a*][j], u_ij = T_j - Z[b][actions][i], h = |u| <= 1 ? (0.5 u) u : |u| - 0.5,
 *                w_ij = |tau_i - 1{u_ij < 0}|, tau_i = (i + 0.5) / N, L_b = sum_i (sum_j w_ij h_ij) / N,
 *                dz[b][actions N + i] = weights_b (-(sum_j w_ij clamp(u_ij, -1, 1)) / N) / B
 *   categorical  p' = softmax(z_next[a*][:]), Tz_k = clamp(returns + live z_k, v_min, v_max),
 *                m_i = sum_k p'_k max(0, 1 - |Tz_k - z_i| / D), L_b = -sum_i m_i log p_i, p = softmax(Z[b][actions][:]),
 *                dz[b][actions N + i] = weights_b (p_i sum(m) - m_i) / B
 *   loss = (sum_b weights_b L_b) / B; every other column of dz is written as zero; sample_loss_b = L_b (no weight).
 * The quantile arithmetic is separately rounded fp32 in a fixed order; no floating-point atomics anywhere,
 * so both losses are bit-reproducible and a sample's result depends on the batch only through the final / B.
 * Conventions of the `_dev` sections: arguments are checked on the host before any handle is read (QLX_E_INVALID, the field
 * named), everything is enqueued on the model's stream, no call allocates, synchronises or copies to the host; n and batch
 * are bounded by qlx_model_reserve (QLX_E_STATE above it).  An action or a_star >= 3 is treated as 0 and sets the model's
 * sticky flag (qlx_model_sync reports it once); non-finite inputs propagate. */
#define QLX_DIST_QUANTILE 0
#define QLX_DIST_CATEGORICAL 1
#define QLX_DIST_MAX_ATOMS 341
typedef struct qlx_dist {
  int32_t kind;            /* QLX_DIST_QUANTILE (atoms 1..341) or QLX_DIST_CATEGORICAL (atoms 2..341) */
  uint32_t atoms;
  float v_min, v_max;      /* categorical: finite, v_min < v_max; ignored for quantiles */
} qlx_dist;
typedef struct qlx_dist_batch {      /* device pointers; the first four are what qlx_replay_batch_dev writes */
  const uint8_t* actions;            /* [B] */
  const float* returns;              /* [B] */
  const float* discounts;            /* [B] */
  const uint8_t* terminals;          /* [B] */
  const float* z_next;               /* [B][3 N]: the target net's head output on s' */
  const uint8_t* a_star;             /* [B] or NULL: NULL = first argmax of the values of z_next; else the caller's (double DQN) */
  const float* weights;              /* [B] or NULL */
} qlx_dist_batch;
#ifdef __cplusplus
static_assert(sizeof(qlx_dist) == 16, "qlx_dist ABI size");
static_assert(sizeof(qlx_dist_batch) == 56, "qlx_dist_batch ABI size");
#endif
/* values of n (1..8192) rows d_z [n][3 N]: d_q [n][3], d_actions [n], d_max_q [n]; any may be NULL, not all three */
int32_t qlx_head_values_dev(qlx_head* h, const qlx_dist* dist, const float* d_z, uint32_t n, float* d_q, uint8_t* d_actions,
                            float* d_max_q);
/* one launch for a*, target, L_b and the whole dz row (zeros included), one tiny launch for the scalar loss (skipped when
 * d_loss is NULL).  d_dz [batch][3 N]; d_loss one float; d_sample_loss [batch]; d_a_star_out [batch].  batch 1..4096 */
int32_t qlx_head_dist_loss_dev(qlx_head* h, const qlx_dist* dist, const float* d_z, const qlx_dist_batch* batch_in, uint32_t batch,
                               float* d_dz, float* d_loss_or_null, float* d_sample_loss_or_null, uint8_t* d_a_star_out_or_null);
/* one update: by definition, and bit for bit, qlx_head_forward_dev(src, batch, d_z_work, NULL), qlx_head_dist_loss_dev,
 * qlx_head_backward_dev with that forward's ticket and no dq, qlx_model_step_dev(0).  The two work buffers [batch][3 N] are
 * the caller's and hold Z and dz afterwards. */
int32_t qlx_head_dist_train_dev(qlx_head* h, const qlx_dist* dist, const qlx_states_dev* src, const qlx_dist_batch* batch_in,
                                uint32_t batch, float* d_z_work, float* d_dz_work, float* d_loss_or_null,
                                float* d_sample_loss_or_null);

/* ---- acting with, evaluating and checkpointing a distributional head ----
 * One kernel gives a row's values, first argmax and epsilon-greedy draw: the values are qlx_head_values_dev's bits (the same
 * device functions), the draw is the evaluator's (random when epsilon > 0 and epsilon > the f64 from words 0-1 of the row's
 * stream; the random action uniform over 3 from word 2).  Conventions of the sections above: argument errors (a null head,
 * dist, d_z / d_z_work or d_actions, every qlx_dist error, the source's cases, n 0 or > 8192, an epsilon that is not finite
 * or outside 0..1) are QLX_E_INVALID with the field named, found before any handle is read; then 3 * atoms against the
 * width (QLX_E_INVALID naming atoms), the reserve (QLX_E_STATE) and the source's handles.  A failed call launches nothing.
 * Both calls only enqueue on the model's stream. */
/* epsilon-greedy on given rows d_z [n][3 N]: row r draws from stream (seed, r, step, purpose 9), f64 from word 0, action
 * from word 2.  d_max_q [n] and d_q [n][3] are the greedy values, whatever action was drawn; with epsilon 0 nothing is drawn
 * and d_actions is qlx_head_values_dev's. */
int32_t qlx_head_select_dev(qlx_head* h, const qlx_dist* dist, const float* d_z, uint32_t n, double epsilon, uint64_t seed,
                            uint32_t step, uint8_t* d_actions, float* d_max_q_or_null, float* d_q_or_null);
/* by definition, and bit for bit: qlx_head_forward_dev(src, n, d_z_work, NULL), then qlx_head_select_dev on d_z_work
 * [n][3 N], which holds Z afterwards; every check of both is made before the first launch */
int32_t qlx_head_act_dev(qlx_head* h, const qlx_dist* dist, const qlx_states_dev* src, uint32_t n, double epsilon, uint64_t seed,
                         uint32_t step, uint8_t* d_actions, float* d_max_q_or_null, float* d_q_or_null, float* d_z_work);
/* qlx_evaluator_run (above) with the policy of h read as `dist`: q = the values of Z(obs_e) in place of the built-in Q, all
 * else word for word - the env reset per run, the purpose-8 draws, the records, fp32 sums in step order, retirement,
 * polling, vector_steps, forward_samples, compaction; it runs on the stream of the head's model and synchronises.  Per
 * vector step: the trunk forward over the rows, the head's forward into a Z workspace the evaluator owns ([n_envs][width],
 * allocated before the loop of the first run that needs it, grown only), one select launch; the built-in head is not
 * launched.  qlx_evaluator_episodes serves the last run of either kind.  Argument errors (null ev, h, dist or out, every
 * qlx_dist error) before any handle is read; then 3 * atoms against the width and the devices.  No weight, Adam slot,
 * iteration count, gradient buffer or sticky flag of the model or the head changes; like any forward the run advances the
 * model's forward ticket, so a ticket taken before it is no longer current and a backward given it runs its forward again.
 * The model's workspace grows to n_envs rows if it is smaller: qlx_model_reserve does not bound an evaluation. */
int32_t qlx_evaluator_run_head(qlx_evaluator* ev, qlx_head* h, const qlx_dist* dist, qlx_eval_summary* out);
/* The head's persistence, as qlx_model_write_checkpoint / _read_checkpoint are the model's (host calls, synchronise): magic
 * "QLXHEAD1", two int64 {width, iterations}, then Wh|bh weights, Adam m, Adam v, 513 * width floats each.  A file with
 * another magic, another width or too few bytes is refused with QLX_E_IO and nothing of the head changes.  A read restores
 * iterations too, so a model and a head restored from their two files continue an interrupted run bit for bit. */
int32_t qlx_head_write_checkpoint(qlx_head* h, const char* path);
int32_t qlx_head_read_checkpoint(qlx_head* h, const char* path);

/* ---------------- Prioritized replay on device tensors (beyond the reference) ----------------
 * The learner's proportional prioritized replay (the sum tree above: same heap, same draws, same weights, same priority
 * write) kept inside a qlx_replay and driven one batch per call from device memory.  Conventions of "Device-tensor env and
 * replay calls": arguments are checked on the host before anything is launched, the `_dev` calls enqueue on the replay's
 * stream and neither synchronise, allocate nor copy to the host.
 * Semantics: one fp32 heap of 2L nodes (L = next power of two >= capacity), leaf L + slot = priority^alpha of the PHYSICAL
 * ring slot, node i = t[2i] + t[2i + 1].  A pushed transition enters at per_max (1 at first, then the largest priority
 * ever written).  Draw b of a batch: x = (T / B)(b + r_b), r_b from stream (seed, update_idx, rank, purpose 7, word b),
 * descending left iff x < left or right == 0; weight (len leaf / T)^-beta divided by the batch maximum; the result is the
 * logical index (slot + cap - start) % cap, start = (total - len) % cap.  Draws are with replacement: batch > len is fine.
 * Host checks (QLX_E_INVALID, the field named): a null handle or required pointer, batch 0 or > 4096, n > 4096, beta or
 * alpha not finite or < 0, eps not finite or <= 0, len == 0 for a draw.  After them: priorities not enabled, QLX_E_STATE.
 * Data the host cannot see: an index >= len, or a td_abs that is NaN, infinite or negative, writes nothing (leaf and
 * per_max stay) and sets the replay's sticky flag, which qlx_replay_sync reports as QLX_E_INVALID, once. */
/* Allocates the tree (12 bytes per leaf), gives the len live slots priority 1 and the rest 0, per_max = 1, builds the tree
 * and synchronises; a second call resets to that state.  From here on every push (qlx_replay_push_dev, qlx_replay_push, a
 * learner's) also writes per_max into the pushed slots and rebuilds the tree, on the stream the push runs on; a replay
 * without priorities pushes exactly as before.  Snapshots do not store priorities. */
int32_t qlx_replay_per_enable(qlx_replay* rb);
/* one batch of `batch` (1..4096) draws into d_out_indices [batch] and, unless NULL, d_out_weights [batch] */
int32_t qlx_replay_per_sample_dev(qlx_replay* rb, uint64_t seed, uint32_t update_idx, uint32_t rank, uint32_t batch, float beta,
                                  uint64_t* d_out_indices, float* d_out_weights_or_null);
/* leaf = (td_abs + eps)^alpha for n (0..4096; 0 launches nothing) logical indices; an index that appears more than once
 * keeps the value of its LAST position.  The indices are logical indices as they are NOW: as with qlx_replay_batch_dev,
 * indices drawn before a push on a full ring no longer name the same transitions (each push of n_envs transitions moves
 * every logical index down by n_envs once len == capacity), so write the priorities of a batch before the next push.
 * After the call the tree is consistent: a draw needs no build. */
int32_t qlx_replay_per_update_dev(qlx_replay* rb, const uint64_t* d_indices, const float* d_td_abs, uint32_t n, float alpha,
                                  float eps);
/* read-out for tests and diagnostics (host outputs, any may be NULL; synchronises): the leaves by physical slot
 * [capacity], the whole heap [2L] (node 0 unused), L, the total t[1], per_max and start */
int32_t qlx_replay_per_get(qlx_replay* rb, float* leaves, float* tree, uint32_t* L, float* total, float* per_max, uint64_t* start);

#ifdef __cplusplus
}
#endif
#endif /* QLX_H */
