"""Host-side mirror of the reference's `ql` trait surface over libqlx's C ABI (include/qlx.h).

Names follow the reference so tests read like its own:
  Environment / Action           src/ql/src/prelude.rs:12-63
  BreakoutEnvironment            src/_breakout-ml/src/breakout_environment.rs:131-207   (batched: n envs)
  ReplayBuffer                   src/ql-with-tensorflow/src/learn/replay_buffer.rs:52-138
  DeepQLearningModel             src/ql-with-tensorflow/src/ml_model/model.rs:29-77
  Parameter / SelfDrivingQLearner  src/ql-with-tensorflow/src/learn/self_driving_tf_q_learner.rs:20-139

Everything here is plumbing: the compute runs in libqlx.so (HIP, gfx950).  There is no CPU fallback —
if the library or a GPU is missing, construction raises QlError.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("QLX_LIB_PATH") or os.path.join(_HERE, "lib", "libqlx.so")   # override: A/B builds

ACTION_SPACE = 3           # BreakoutAction::ACTION_SPACE
FRAME = 84
SLOTS = 4
STATE_BYTES = FRAME * FRAME * SLOTS
NUM_VARS = 10
VAR_SHAPES = [(8, 8, 4, 32), (32,), (4, 4, 32, 64), (64,), (3, 3, 64, 64), (64,), (3136, 512), (512,), (512, 3), (3,)]
VAR_NAMES = ["convolution_layer1/kernel", "convolution_layer1/bias", "convolution_layer2/kernel",
             "convolution_layer2/bias", "convolution_layer3/kernel", "convolution_layer3/bias",
             "full_layer/kernel", "full_layer/bias", "action_layer/kernel", "action_layer/bias"]


class QlError(RuntimeError):
    """prelude.rs:70-86 QlError; raised for every non-zero status of the C ABI."""


STATE_DTYPE = np.dtype([
    ("ball_x", "<f4"), ("ball_y", "<f4"), ("dir_x", "<f4"), ("dir_y", "<f4"),
    ("panel_min_x", "<f4"), ("panel_min_y", "<f4"), ("panel_max_x", "<f4"), ("panel_max_y", "<f4"),
    ("panel_speed", "<f4"),
    ("score", "<u4"), ("finished", "<u4"), ("next_slot", "<u4"), ("fault", "<u4"), ("reset_count", "<u4"),
    ("bricks", "<u8"),
])


class Params(C.Structure):
    """qlx_params = Parameter (self_driving_tf_q_learner.rs:20-67) + build fields."""
    _fields_ = [
        ("gamma", C.c_float),
        ("lowest_episode_reward_goal_threshold_pct", C.c_float),
        ("epsilon_max", C.c_double),
        ("epsilon_min", C.c_double),
        ("epsilon_greedy_steps", C.c_double),
        ("max_steps_per_episode", C.c_uint64),
        ("epsilon_pure_random_steps", C.c_uint64),
        ("history_buffer_len", C.c_uint64),
        ("update_after_actions", C.c_uint64),
        ("target_sync_steps", C.c_uint64),
        ("episode_reward_history_buffer_len", C.c_uint64),
        ("n_envs", C.c_uint32),
        ("batch_size", C.c_uint32),
        ("env_seed", C.c_uint64),
        ("learner_seed", C.c_uint64),
        ("init_seed", C.c_uint64),
        ("rank", C.c_uint32),
        ("flags", C.c_uint32),
        ("per_alpha", C.c_float),
        ("per_beta", C.c_float),
        ("per_eps", C.c_float),
        ("qnet_precision", C.c_uint32),
        ("stats_after_steps", C.c_uint64),
        ("checkpoint_file", C.c_char * 256),
        ("episode_reward_goal", C.c_float),
        ("n_step", C.c_uint32),   # n-step returns: 0 / 1 = the reference's 1-step target, 2..NSTEP_MAX = n-step
    ]

NSTEP_MAX = 32  # QLX_NSTEP_MAX
DOUBLE_DQN = 1
PER = 2
PREC_F32 = 0    # QLX_PREC_F32: the reference's fp32 arithmetic (bit-exact against the oracle)
PREC_BF16 = 1   # QLX_PREC_BF16: bf16 MFMA operands, fp32 accumulation (the labelled fast path)
ARCH_F32 = 1    # QLX_ARCH_NATURE_DQN
ARCH_BF16 = 2   # QLX_ARCH_NATURE_DQN_BF16


class LearnerStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("step_count", "vec_steps", "update_count", "episode_count",
                                          "replay_len", "solved")] + [
        ("epsilon", C.c_double), ("running_reward", C.c_float), ("last_loss", C.c_float)]


class EvalConfig(C.Structure):
    """qlx_eval_config (policy evaluation, beyond the reference)"""
    _fields_ = [("n_envs", C.c_uint32), ("episodes_per_env", C.c_uint32), ("max_steps_per_episode", C.c_uint64),
                ("epsilon", C.c_double), ("env_seed", C.c_uint64), ("policy_seed", C.c_uint64),
                ("poll_steps", C.c_uint32), ("flags", C.c_uint32)]


class EvalSummary(C.Structure):
    """qlx_eval_summary"""
    _fields_ = [(k, C.c_uint64) for k in ("episodes", "env_steps", "vector_steps", "forward_samples",
                                          "terminal_episodes")] + [
        ("action_counts", C.c_uint64 * 3), ("mean_return", C.c_double), ("mean_length", C.c_double),
        ("mean_max_q", C.c_double), ("min_return", C.c_float), ("max_return", C.c_float)]


EVAL_MAX_ENVS = 8192   # QLX_EVAL_MAX_ENVS

SNAPSHOT_VERSION = 1      # QLX_SNAPSHOT_VERSION
SNAPSHOT_LEARNER = 1      # QLX_SNAPSHOT_LEARNER
SNAPSHOT_REPLAY = 2       # QLX_SNAPSHOT_REPLAY
FRAME_CODEC_RAW = 0       # QLX_FRAME_CODEC_RAW
FRAME_CODEC_BITMAP = 1    # QLX_FRAME_CODEC_BITMAP: a bitmap of each frame's non-zero bytes + those bytes
FRAME_BYTES = FRAME * FRAME


class SnapshotInfo(C.Structure):
    """qlx_snapshot_info (snapshots, beyond the reference)"""
    _fields_ = [(k, C.c_uint32) for k in ("format_version", "kind", "frame_codec", "reserved")] + [
        (k, C.c_uint64) for k in ("step_count", "vec_steps", "update_count", "episode_count", "replay_len",
                                  "replay_total", "frames", "frame_bytes_raw", "frame_bytes_stored", "file_bytes")] + [
        ("params", Params)]


class UpdateMetrics(C.Structure):
    """qlx_update_metrics: one row per training update (training metrics, beyond the reference)"""
    _fields_ = [("update", C.c_uint64), ("step_count", C.c_uint64)] + [
        (k, C.c_uint32) for k in ("batch", "n_actions", "n_vars", "n_clipped", "n_linear", "n_nonfinite")] + [
        (k, C.c_float) for k in ("loss", "q_taken_mean", "q_taken_min", "q_taken_max", "q_max_mean", "action_gap_mean",
                                 "y_mean", "y_min", "y_max", "td_abs_mean", "td_abs_max", "weight_mean",
                                 "grad_norm_global")] + [
        ("reserved", C.c_uint32), ("argmax_counts", C.c_uint32 * 8), ("grad_norm", C.c_float * 16),
        ("td_hist", C.c_uint32 * 16)]


class BatchDev(C.Structure):
    """qlx_batch_dev: the device pointers qlx_replay_batch_dev writes (any may be None)"""
    _fields_ = [(k, C.c_void_p) for k in ("s", "s_next", "actions", "returns", "discounts", "terminals", "last_indices",
                                          "steps")]


class StatesDev(C.Structure):
    """qlx_states_dev: the one state source of a qlx_model_*_dev call (obs, or replay + indices, or env), the channel
    order the net sees (OBS_*) and, for the replay source, which state of the transition (0 = s, 1 = s')"""
    _fields_ = [("obs", C.c_void_p), ("replay", C.c_void_p), ("indices", C.c_void_p), ("env", C.c_void_p),
                ("layout", C.c_int32), ("which", C.c_int32)]


class Dist(C.Structure):
    """qlx_dist: how a head of width 3 * atoms is read: kind DIST_QUANTILE (atoms 1..341) or
    DIST_CATEGORICAL (atoms 2..341, finite v_min < v_max)"""
    _fields_ = [("kind", C.c_int32), ("atoms", C.c_uint32), ("v_min", C.c_float), ("v_max", C.c_float)]


class DistBatch(C.Structure):
    """qlx_dist_batch: device pointers [B] of a distributional loss's batch; the first four are what qlx_replay_batch_dev
    writes, z_next is [B][3 atoms], a_star and weights may be None"""
    _fields_ = [(k, C.c_void_p) for k in ("actions", "returns", "discounts", "terminals", "z_next", "a_star", "weights")]


DIST_QUANTILE = 0       # QLX_DIST_QUANTILE
DIST_CATEGORICAL = 1    # QLX_DIST_CATEGORICAL
DIST_MAX_ATOMS = 341    # QLX_DIST_MAX_ATOMS
OBS_NHWC_SLOT = 0   # QLX_OBS_NHWC_SLOT: [n][84][84][4] (x, y, ring slot)
OBS_NCHW_TIME = 1   # QLX_OBS_NCHW_TIME: [n][4][84][84] (age, x, y), channel 0 oldest
STEP_GRADS_WRITTEN = 1   # QLX_STEP_GRADS_WRITTEN: qlx_model_step_dev after the caller wrote the gradient buffer
HEAD_IN = 512            # the wide head's input: a4, the ReLU output of fc1
HEAD_MAX_WIDTH = 1024    # QLX_HEAD_MAX_WIDTH
P_ACT_DEV = 9            # the Philox purpose of qlx_head_select_dev / _act_dev's draws (P_EVAL = 8 is the evaluator's)

_NP_OF_C = {C.c_uint64: "<u8", C.c_uint32: "<u4", C.c_float: "<f4"}
# the same row as a numpy structured dtype (what metrics() returns an array of)
UPDATE_METRICS_DTYPE = np.dtype([(k, _NP_OF_C[t]) if t in _NP_OF_C else (k, _NP_OF_C[t._type_], (t._length_,))
                                 for k, t in UpdateMetrics._fields_])


def metrics_td_bin(x):
    """the td_hist bin of |td| = x (qlx_metrics_td_bin, host only): the function the metrics kernel uses"""
    return int(lib().qlx_metrics_td_bin(C.c_float(x)))


class _Metrics:
    """Per-update training metrics of a learner handle (qlx_*_metrics_enable / _info / _read)"""

    def metrics_enable(self, capacity):
        """a ring of `capacity` rows in device memory, one row per update from now on; 0 turns metrics off"""
        _check(getattr(lib(), self._prefix + "_metrics_enable")(self.h, capacity))

    def metrics_info(self):
        """dict(capacity, recorded, unread) from host counters (no synchronisation)"""
        cap, rec, unread = C.c_uint32(), C.c_uint64(), C.c_uint64()
        _check(getattr(lib(), self._prefix + "_metrics_info")(self.h, C.byref(cap), C.byref(rec), C.byref(unread)))
        return dict(capacity=cap.value, recorded=rec.value, unread=unread.value)

    def metrics(self, max_rows=None):
        """(rows, dropped): the unread rows, oldest first, as an array of UPDATE_METRICS_DTYPE (all of them, or at most
        max_rows) and how many unread rows were overwritten since the previous call; synchronises"""
        cap = self.metrics_info()["unread"] if max_rows is None else int(max_rows)
        rows = np.zeros(max(cap, 1), UPDATE_METRICS_DTYPE)
        n, dropped = C.c_uint64(), C.c_uint64()
        _check(getattr(lib(), self._prefix + "_metrics_read")(self.h, _p(rows), cap, C.byref(n), C.byref(dropped)))
        return rows[:n.value], dropped.value


def _eval_config(n_envs, episodes_per_env=1, max_steps_per_episode=10_000, epsilon=0.0, env_seed=0x51A5EED,
                 policy_seed=1, poll_steps=0, flags=0):
    return EvalConfig(n_envs=n_envs, episodes_per_env=episodes_per_env, max_steps_per_episode=max_steps_per_episode,
                      epsilon=epsilon, env_seed=env_seed, policy_seed=policy_seed, poll_steps=poll_steps, flags=flags)


def _eval_summary(s):
    d = {k: getattr(s, k) for k, _ in EvalSummary._fields_}
    d["action_counts"] = np.array(list(s.action_counts), np.uint64)
    return d


def Parameter(**kw):
    """Parameter::default() with overrides (self_driving_tf_q_learner.rs:50-67)."""
    p = Params(gamma=0.99, lowest_episode_reward_goal_threshold_pct=0.9, epsilon_max=1.0, epsilon_min=0.1,
               epsilon_greedy_steps=1_000_000.0, max_steps_per_episode=10_000, epsilon_pure_random_steps=50_000,
               history_buffer_len=1_000_000, update_after_actions=4, target_sync_steps=0,
               episode_reward_history_buffer_len=100, n_envs=1, batch_size=32, env_seed=0x51A5EED, learner_seed=1,
               init_seed=2, rank=0, flags=0, per_alpha=0.6, per_beta=0.4, per_eps=1e-6, qnet_precision=PREC_F32,
               stats_after_steps=25_000, checkpoint_file=b"", episode_reward_goal=float("nan"), n_step=1)
    for k, v in kw.items():
        if k == "checkpoint_file" and isinstance(v, str):
            v = v.encode()
        setattr(p, k, v)
    return p


_lib = None


def lib():
    """Load libqlx.so (fails loudly: the product has no CPU path)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise QlError(f"{LIB_PATH} not built — run `make lib` (or __graft_entry__.build())")
    L = C.CDLL(LIB_PATH)
    vp, u8p = C.c_void_p, C.c_void_p
    i32, u32, u64, f32 = C.c_int32, C.c_uint32, C.c_uint64, C.c_float
    sig = {
        "qlx_last_error": ([], C.c_char_p), "qlx_version": ([], i32),
        "qlx_env_action_space": ([i32], i32), "qlx_env_reward_goal_mean": ([i32], f32),
        "qlx_env_create": ([i32, u32, u64, i32, C.POINTER(vp)], i32), "qlx_env_destroy": ([vp], i32),
        "qlx_env_count": ([vp], u32), "qlx_env_reset": ([vp, u8p], i32), "qlx_env_step": ([vp, u8p, vp, u8p], i32),
        "qlx_env_step_dev": ([vp, vp, vp, vp], i32), "qlx_env_obs": ([vp, u8p], i32),
        "qlx_env_states": ([vp, vp], i32), "qlx_env_hashes": ([vp, vp], i32), "qlx_env_sync": ([vp], i32),
        "qlx_env_set_states": ([vp, vp], i32), "qlx_env_episode_steps": ([vp, vp], i32),
        "qlx_replay_create": ([u64, u32, i32, C.POINTER(vp)], i32), "qlx_replay_destroy": ([vp], i32),
        "qlx_replay_len": ([vp], u64), "qlx_replay_push_dev": ([vp, vp, vp, vp, vp], i32),
        "qlx_replay_push": ([vp, vp, vp, vp, vp], i32),
        "qlx_replay_sample_distinct": ([vp, u64, u32, u32, u32, vp], i32),
        "qlx_replay_get_many": ([vp, vp, u32, vp, vp, vp, vp, vp], i32),
        "qlx_replay_nstep": ([vp, vp, u32, u32, f32, vp, vp, vp, vp, vp], i32),
        # device-tensor calls (qlx_torch.py is their caller)
        "qlx_env_stream": ([vp, C.POINTER(vp)], i32), "qlx_replay_stream": ([vp, C.POINTER(vp)], i32),
        "qlx_replay_share_stream": ([vp, vp], i32), "qlx_replay_sync": ([vp], i32),
        "qlx_env_obs_dev": ([vp, i32, vp], i32), "qlx_env_reset_dev": ([vp, vp], i32),
        "qlx_replay_sample_distinct_dev": ([vp, u64, u32, u32, u32, vp], i32),
        "qlx_replay_batch_dev": ([vp, vp, u32, u32, f32, i32, C.POINTER(BatchDev)], i32),
        "qlx_replay_per_enable": ([vp], i32),
        "qlx_replay_per_sample_dev": ([vp, u64, u32, u32, u32, f32, vp, vp], i32),
        "qlx_replay_per_update_dev": ([vp, vp, vp, u32, f32, f32], i32),
        "qlx_replay_per_get": ([vp, vp, vp, vp, vp, vp, vp], i32),
        "qlx_model_create": ([i32, u64, i32, C.POINTER(vp)], i32), "qlx_model_destroy": ([vp], i32),
        "qlx_model_num_vars": ([], i32), "qlx_model_var_size": ([i32], C.c_int64), "qlx_model_hparams": ([vp], i32),
        "qlx_bg_model_hparams": ([vp], i32),
        "qlx_model_get_var": ([vp, i32, i32, vp], i32), "qlx_model_set_var": ([vp, i32, i32, vp], i32),
        "qlx_model_iterations": ([vp], C.c_int64), "qlx_model_copy_weights": ([vp, vp], i32),
        "qlx_model_predict": ([vp, vp, u32, vp, vp], i32), "qlx_model_batch_max_q": ([vp, vp, u32, vp], i32),
        "qlx_model_train": ([vp, vp, vp, vp, u32, vp, vp, vp], i32),
        "qlx_model_apply_gradient": ([vp, vp, C.c_float, vp], i32),
        "qlx_model_last_activation": ([vp, i32, vp], i32),
        "qlx_model_write_checkpoint": ([vp, C.c_char_p], i32), "qlx_model_read_checkpoint": ([vp, C.c_char_p], i32),
        "qlx_model_sync": ([vp], i32),
        # the Q-net on device tensors (qlx_torch.TorchQNet is their caller)
        "qlx_model_stream": ([vp, C.POINTER(vp)], i32), "qlx_model_share_stream": ([vp, vp], i32),
        "qlx_model_reserve": ([vp, u32], i32),
        "qlx_model_q_dev": ([vp, C.POINTER(StatesDev), u32, vp, vp, vp], i32),
        "qlx_model_train_dev": ([vp, C.POINTER(StatesDev), vp, vp, vp, u32, vp, vp], i32),
        "qlx_model_copy_weights_dev": ([vp, vp], i32),
        "qlx_model_forward_ticket": ([vp, C.POINTER(C.c_uint64)], i32),
        "qlx_model_backward_dev": ([vp, C.POINTER(StatesDev), vp, u32, u64], i32),
        "qlx_model_step_dev": ([vp, u32], i32),
        "qlx_model_grads_dev": ([vp, C.POINTER(vp), C.POINTER(C.c_uint64)], i32),
        # the wide output head (WideHead; qlx_torch.TorchQNet.attach_head)
        "qlx_head_create": ([vp, u32, u64, C.POINTER(vp)], i32), "qlx_head_destroy": ([vp], i32),
        "qlx_head_width": ([vp], i32), "qlx_head_iterations": ([vp], C.c_int64),
        "qlx_head_get_var": ([vp, i32, i32, vp], i32), "qlx_head_set_var": ([vp, i32, i32, vp], i32),
        "qlx_head_forward_dev": ([vp, C.POINTER(StatesDev), u32, vp, vp], i32),
        "qlx_head_backward_dev": ([vp, C.POINTER(StatesDev), vp, vp, u32, u64], i32),
        "qlx_head_grads_dev": ([vp, C.POINTER(vp), C.POINTER(C.c_uint64)], i32),
        "qlx_head_copy_weights_dev": ([vp, vp], i32),
        # distributional losses on the wide head (qlx_torch.TorchQNet.head_values / dist_loss / train_dist)
        "qlx_head_values_dev": ([vp, C.POINTER(Dist), vp, u32, vp, vp, vp], i32),
        "qlx_head_dist_loss_dev": ([vp, C.POINTER(Dist), vp, C.POINTER(DistBatch), u32, vp, vp, vp, vp], i32),
        "qlx_head_dist_train_dev": ([vp, C.POINTER(Dist), C.POINTER(StatesDev), C.POINTER(DistBatch), u32, vp, vp, vp, vp], i32),
        # acting with, evaluating and checkpointing a distributional head (TorchQNet.select / act / evaluate / save_head)
        "qlx_head_select_dev": ([vp, C.POINTER(Dist), vp, u32, C.c_double, u64, u32, vp, vp, vp], i32),
        "qlx_head_act_dev": ([vp, C.POINTER(Dist), C.POINTER(StatesDev), u32, C.c_double, u64, u32, vp, vp, vp, vp], i32),
        "qlx_evaluator_run_head": ([vp, vp, C.POINTER(Dist), C.POINTER(EvalSummary)], i32),
        "qlx_head_write_checkpoint": ([vp, C.c_char_p], i32), "qlx_head_read_checkpoint": ([vp, C.c_char_p], i32),
        "qlx_params_default": ([vp], None),
        "qlx_learner_create": ([C.POINTER(Params), i32, C.POINTER(vp)], i32), "qlx_learner_destroy": ([vp], i32),
        "qlx_learner_vector_step": ([vp], i32), "qlx_learner_run": ([vp, u64], i32), "qlx_learner_sync": ([vp], i32),
        "qlx_learner_prefill": ([vp, u64], i32), "qlx_learner_end_episodes": ([vp, vp], i32), "qlx_learner_stats_events": ([vp], u64),
        "qlx_learner_learn_till_mastered": ([vp, u64, C.POINTER(u64)], i32),
        "qlx_learner_last_log": ([vp, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)], i32),
        "qlx_learner_stats_get": ([vp, C.POINTER(LearnerStats)], i32),
        "qlx_learner_last": ([vp, vp, vp, vp, vp, vp, vp, C.POINTER(u32)], i32),
        "qlx_learner_env": ([vp], vp), "qlx_learner_replay": ([vp], vp), "qlx_learner_model": ([vp, i32], vp),
        "qlx_learner_priorities": ([vp, vp, vp, vp], i32),
        "qlx_metrics_td_bin": ([f32], i32),
        "qlx_learner_metrics_enable": ([vp, u32], i32), "qlx_bg_learner_metrics_enable": ([vp, u32], i32),
        "qlx_learner_metrics_info": ([vp, C.POINTER(u32), C.POINTER(u64), C.POINTER(u64)], i32),
        "qlx_bg_learner_metrics_info": ([vp, C.POINTER(u32), C.POINTER(u64), C.POINTER(u64)], i32),
        "qlx_learner_metrics_read": ([vp, vp, u64, C.POINTER(u64), C.POINTER(u64)], i32),
        "qlx_bg_learner_metrics_read": ([vp, vp, u64, C.POINTER(u64), C.POINTER(u64)], i32),
        "qlx_learner_frame_sparsity": ([vp, vp], i32),
        "qlx_learner_action_counts": ([vp, vp], i32), "qlx_bg_learner_action_counts": ([vp, vp], i32),
        "qlx_learner_episode_rewards": ([vp, vp, u64, C.POINTER(u64)], i32),
        "qlx_bg_learner_episode_rewards": ([vp, vp, u64, C.POINTER(u64)], i32),
        "qlx_learner_update_log": ([vp, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)], i32),
        "qlx_bg_learner_update_log": ([vp, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)], i32),
        "qlx_evaluator_create": ([C.POINTER(EvalConfig), i32, C.POINTER(vp)], i32), "qlx_evaluator_destroy": ([vp], i32),
        "qlx_evaluator_run": ([vp, vp, C.POINTER(EvalSummary)], i32),
        "qlx_evaluator_episodes": ([vp, vp, vp, vp, vp], i32), "qlx_evaluator_env": ([vp], vp),
        "qlx_learner_evaluate": ([vp, C.POINTER(EvalConfig), C.POINTER(EvalSummary)], i32),
        "qlx_snapshot_info_read": ([C.c_char_p, C.POINTER(SnapshotInfo)], i32),
        "qlx_learner_save": ([vp, C.c_char_p], i32), "qlx_learner_load": ([C.c_char_p, i32, C.POINTER(vp)], i32),
        "qlx_replay_save": ([vp, C.c_char_p], i32), "qlx_replay_load": ([C.c_char_p, i32, C.POINTER(vp)], i32),
        "qlx_frame_codec_roundtrip": ([vp, u32, i32, i32, vp, u64, C.POINTER(u64), vp], i32),
        "qlx_dbscan_f32": ([vp, u64, C.c_float, u64, vp, C.POINTER(u64)], i32),
        "qlx_dbscan_f32_format": ([vp, u64, C.c_float, u64, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)], i32),
        "qlx_sumtree_create": ([u64, i32, C.POINTER(vp)], i32), "qlx_sumtree_destroy": ([vp], i32),
        "qlx_sumtree_set_leaves": ([vp, vp], i32), "qlx_sumtree_get": ([vp, vp, vp, vp], i32),
        "qlx_sumtree_sample": ([vp, u64, u32, u32, u32, u64, C.c_float, u32, vp, vp], i32),
        "qlx_sumtree_update": ([vp, vp, vp, u32, C.c_float, C.c_float], i32),
        "qlx_dist_unique_id": ([vp], i32), "qlx_learner_dist_init": ([vp, i32, i32, vp], i32),
        "qlx_learner_comm_size": ([vp, vp], i32),
        "qlx_learner_profile": ([vp, i32], i32),
        "qlx_learner_profile_get": ([vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(u64)], i32),
        "qlx_learner_profile_filter": ([vp, C.c_char_p], i32),
        "qlx_learner_profile_sample": ([vp, C.c_char_p, u32], i32),
        "qlx_learner_profile_names": ([vp, C.c_char_p, C.c_size_t], i32),
        # BallGame
        "qlx_bg_env_create": ([u32, u64, i32, C.POINTER(vp)], i32), "qlx_bg_env_destroy": ([vp], i32),
        "qlx_bg_env_reset": ([vp, u8p], i32), "qlx_bg_env_step": ([vp, u8p, vp, u8p], i32),
        "qlx_bg_env_obs": ([vp, u8p], i32), "qlx_bg_env_states": ([vp, vp], i32), "qlx_bg_env_set_states": ([vp, vp], i32),
        "qlx_bg_model_create": ([u64, i32, C.POINTER(vp)], i32), "qlx_bg_model_destroy": ([vp], i32),
        "qlx_bg_model_var_size": ([i32], C.c_int64), "qlx_bg_model_get_var": ([vp, i32, i32, vp], i32),
        "qlx_bg_model_set_var": ([vp, i32, i32, vp], i32), "qlx_bg_model_iterations": ([vp], C.c_int64),
        "qlx_bg_model_predict": ([vp, vp, u32, vp, vp], i32), "qlx_bg_model_batch_max_q": ([vp, vp, u32, vp], i32),
        "qlx_bg_model_train": ([vp, vp, vp, vp, u32, vp, vp, vp], i32),
        "qlx_bg_learner_create": ([C.POINTER(Params), i32, C.POINTER(vp)], i32), "qlx_bg_learner_destroy": ([vp], i32),
        "qlx_bg_learner_run": ([vp, u64], i32), "qlx_bg_learner_sync": ([vp], i32),
        "qlx_bg_learner_stats_get": ([vp, C.POINTER(LearnerStats)], i32),
        "qlx_bg_learner_last": ([vp, vp, vp, vp, vp, vp, vp, C.POINTER(u32)], i32),
        "qlx_bg_learner_env": ([vp], vp), "qlx_bg_learner_model": ([vp, i32], vp),
        "qlx_bg_learner_priorities": ([vp, vp, vp, vp], i32),
        "qlx_bg_model_load_tf": ([vp, C.c_char_p], i32), "qlx_model_load_tf": ([vp, C.c_char_p], i32),
        "qlx_tf_bundle_open": ([C.c_char_p, C.POINTER(vp)], i32), "qlx_tf_bundle_close": ([vp], i32),
        "qlx_tf_bundle_count": ([vp], i32),
        "qlx_tf_bundle_entry": ([vp, i32, C.c_char_p, C.c_size_t, C.POINTER(i32), vp, C.POINTER(i32), C.POINTER(C.c_int64)], i32),
        "qlx_tf_bundle_read": ([vp, C.c_char_p, vp, C.c_size_t], i32),
    }
    for name, (args, res) in sig.items():
        fn = getattr(L, name, None)
        if fn is None:
            continue
        fn.argtypes = args
        fn.restype = res
    _lib = L
    return L


def _text(fn, *args):
    n = C.c_size_t()
    _check(fn(*args, None, 0, C.byref(n)))
    buf = C.create_string_buffer(n.value + 1)
    _check(fn(*args, buf, n.value + 1, C.byref(n)))
    return buf.raw[:n.value].decode("utf-8")


def cluster_analysis(elements, max_neighbor_distance, core_point_min_neighbors):
    """dbscan::cluster_analysis (dbscan.rs:209-262) over f32 values: (clusters as index lists ordered by their lowest
    member, noise indices)"""
    x = np.ascontiguousarray(elements, dtype=np.float32)
    labels = np.zeros(x.shape[0], np.int32)
    nc = C.c_uint64()
    _check(lib().qlx_dbscan_f32(_p(x), x.shape[0], max_neighbor_distance, core_point_min_neighbors, _p(labels), C.byref(nc)))
    clusters = [np.flatnonzero(labels == c).tolist() for c in range(nc.value)]
    return clusters, np.flatnonzero(labels < 0).tolist()


def cluster_analysis_text(elements, max_neighbor_distance, core_point_min_neighbors):
    """Display of the ClusterAnalysisResult<f32> (dbscan.rs:91-133)"""
    x = np.ascontiguousarray(elements, dtype=np.float32)
    return _text(lib().qlx_dbscan_f32_format, _p(x), x.shape[0], max_neighbor_distance, core_point_min_neighbors)


class _LearningStats:
    """learning_update_log (self_driving_tf_q_learner.rs:235-273) for a learner handle"""
    _prefix = "qlx_learner"

    def action_counts(self):
        out = np.zeros(self._n_actions, np.uint64)
        _check(getattr(lib(), self._prefix + "_action_counts")(self.h, _p(out)))
        return out

    def episode_rewards(self):
        n = C.c_uint64()
        fn = getattr(lib(), self._prefix + "_episode_rewards")
        _check(fn(self.h, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.float32)
        _check(fn(self.h, _p(out), n.value, C.byref(n)))
        return out

    def learning_update_log(self):
        return _text(getattr(lib(), self._prefix + "_update_log"), self.h)


def model_hparams(ballgame=False):
    """(learning_rate, beta_1, beta_2, epsilon, clipnorm) every model is created with (float32, no device needed)"""
    out = np.zeros(5, np.float32)
    _check((lib().qlx_bg_model_hparams if ballgame else lib().qlx_model_hparams)(_p(out)))
    return out


def snapshot_info(path):
    """qlx_snapshot_info of a snapshot file as a dict (`params` is a Params); reads the file on the host, no device"""
    info = SnapshotInfo()
    _check(lib().qlx_snapshot_info_read(os.fspath(path).encode(), C.byref(info)))
    d = {k: getattr(info, k) for k, _ in SnapshotInfo._fields_ if k != "params"}
    d["params"] = Params.from_buffer_copy(info.params)
    return d


def frame_codec_roundtrip(frames, codec=FRAME_CODEC_BITMAP, device=0):
    """Test hook of the snapshot frame codec: frames [n][7056] u8 are packed on the GPU, brought to the host, sent back
    and unpacked; (packed bytes as a u8 array, the unpacked frames)"""
    x = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1, FRAME_BYTES)
    n = x.shape[0]
    cap = n * (FRAME_BYTES + FRAME_BYTES // 8) + 16 * (n // 512 + 1) + 2 * n + 64   # the worst case: every byte non-zero
    packed = np.zeros(cap, np.uint8)
    out = np.zeros_like(x)
    nb = C.c_uint64()
    _check(lib().qlx_frame_codec_roundtrip(_p(x), n, codec, device, _p(packed), cap, C.byref(nb), _p(out)))
    return packed[:nb.value].copy(), out


def exported_symbols():
    return [n for n in dir(lib()) if n.startswith("qlx_")]


def _check(status):
    if status != 0:
        msg = lib().qlx_last_error()
        raise QlError(f"qlx status {status}: {msg.decode() if msg else ''}")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class BreakoutEnvironment:
    """Batched `impl Environment for BreakoutEnvironment` on one MI355X (n independent envs)."""

    ACTION_SPACE = ACTION_SPACE

    def __init__(self, n_envs=1, seed=0x51A5EED, device=0, handle=None):
        self._owned = handle is None
        if handle is None:
            h = C.c_void_p()
            _check(lib().qlx_env_create(1, n_envs, seed, device, C.byref(h)))
            handle = h.value
        self.h = handle
        self.n = lib().qlx_env_count(self.h)

    def close(self):
        if getattr(self, "_owned", False) and getattr(self, "h", None):
            lib().qlx_env_destroy(self.h)
        self.h = None

    __del__ = close

    def reset(self, mask=None):
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        _check(lib().qlx_env_reset(self.h, _p(m)))

    def step(self, actions):
        a = np.ascontiguousarray(np.broadcast_to(actions, (self.n,)), dtype=np.uint8)
        r = np.zeros(self.n, np.float32)
        d = np.zeros(self.n, np.uint8)
        _check(lib().qlx_env_step(self.h, _p(a), _p(r), _p(d)))
        return self.state(), r, d.astype(bool)

    def state(self):
        """Reference tensor view [n][x][y][slot] u8 (ToMultiDimArray)."""
        out = np.zeros((self.n, FRAME, FRAME, SLOTS), np.uint8)
        _check(lib().qlx_env_obs(self.h, _p(out)))
        return out

    def mechanics(self):
        out = np.zeros(self.n, STATE_DTYPE)
        _check(lib().qlx_env_states(self.h, _p(out)))
        return out

    def set_mechanics(self, st):
        """Directed start states: STATE_DTYPE[n] over the mechanics (floats as given); episode steps are zeroed,
        ring frames and checksums stay.  finished > 1, next_slot > 3 or bricks >= 2**60 is an error, nothing written."""
        a = np.ascontiguousarray(st, dtype=STATE_DTYPE)
        assert a.shape == (self.n,)
        _check(lib().qlx_env_set_states(self.h, _p(a)))

    def episode_steps(self):
        out = np.zeros(self.n, np.uint32)
        _check(lib().qlx_env_episode_steps(self.h, _p(out)))
        return out

    def hashes(self):
        out = np.zeros(self.n, np.uint64)
        _check(lib().qlx_env_hashes(self.h, _p(out)))
        return out

    @staticmethod
    def episode_reward_goal_mean():
        return lib().qlx_env_reward_goal_mean(1)


class ReplayBuffer:
    def __init__(self, capacity, n_envs, device=0, handle=None):
        self._owned = handle is None
        if handle is None:
            h = C.c_void_p()
            _check(lib().qlx_replay_create(capacity, n_envs, device, C.byref(h)))
            handle = h.value
        self.h = handle
        self.capacity = capacity or None   # unknown for a wrapped handle

    def close(self):
        if getattr(self, "_owned", False) and getattr(self, "h", None):
            lib().qlx_replay_destroy(self.h)
        self.h = None

    __del__ = close

    def __len__(self):
        return int(lib().qlx_replay_len(self.h))

    def add(self, env, actions, rewards, dones):
        """ReplayBuffer::add for the transition every env of `env` just made (replay_buffer.rs:85-98)."""
        a = np.ascontiguousarray(actions, dtype=np.uint8)
        r = np.ascontiguousarray(rewards, dtype=np.float32)
        d = np.ascontiguousarray(dones, dtype=np.uint8)
        _check(lib().qlx_replay_push(self.h, env.h, _p(a), _p(r), _p(d)))

    def sample_distinct(self, seed, update_idx, batch, rank=0):
        out = np.zeros(batch, np.uint64)
        _check(lib().qlx_replay_sample_distinct(self.h, seed, update_idx, rank, batch, _p(out)))
        return out

    def get_many(self, indices):
        idx = np.ascontiguousarray(indices, dtype=np.uint64)
        B = idx.size
        s = np.zeros((B, FRAME, FRAME, SLOTS), np.uint8)
        sn = np.zeros_like(s)
        a = np.zeros(B, np.uint8)
        r = np.zeros(B, np.float32)
        d = np.zeros(B, np.uint8)
        _check(lib().qlx_replay_get_many(self.h, _p(idx), B, _p(s), _p(sn), _p(a), _p(r), _p(d)))
        return dict(state=s, state_next=sn, action=a, reward=r, done=d.astype(bool))

    def save(self, path):
        """the replay alone to a snapshot file (qlx_replay_save)"""
        _check(lib().qlx_replay_save(self.h, os.fspath(path).encode()))

    @classmethod
    def load(cls, path, device=0):
        """a replay created from a file ReplayBuffer.save wrote"""
        h = C.c_void_p()
        _check(lib().qlx_replay_load(os.fspath(path).encode(), device, C.byref(h)))
        rb = cls(0, 0, handle=h.value)
        rb._owned = True
        return rb

    def nstep(self, indices, n_step, gamma):
        """n-step return windows of the transitions at `indices` (qlx_replay_nstep): returns = sum_{j<m} gamma^j r_j,
        discounts = gamma^m, last_indices = logical index of each window's last transition, terminals = its done,
        steps = m <= n_step."""
        idx = np.ascontiguousarray(indices, dtype=np.uint64)
        B = idx.size
        ret = np.zeros(B, np.float32)
        disc = np.zeros(B, np.float32)
        last = np.zeros(B, np.uint64)
        term = np.zeros(B, np.uint8)
        steps = np.zeros(B, np.uint32)
        _check(lib().qlx_replay_nstep(self.h, _p(idx), B, n_step, gamma, _p(ret), _p(disc), _p(last), _p(term), _p(steps)))
        return dict(returns=ret, discounts=disc, last_indices=last, terminals=term.astype(bool), steps=steps)

    # prioritized replay on device tensors (include/qlx.h); the d_* arguments are device addresses
    def per_enable(self):
        """priorities on: every live slot at 1, per_max = 1 (again: reset to that); pushes keep the tree from here on"""
        _check(lib().qlx_replay_per_enable(self.h))

    def per_sample_dev(self, seed, update_idx, batch, beta, d_out_indices, d_out_weights=None, rank=0):
        _check(lib().qlx_replay_per_sample_dev(self.h, seed, update_idx, rank, batch, beta, d_out_indices, d_out_weights))

    def per_update_dev(self, d_indices, d_td_abs, n, alpha, eps):
        _check(lib().qlx_replay_per_update_dev(self.h, d_indices, d_td_abs, n, alpha, eps))

    def per_get(self):
        """dict(leaves [capacity] by physical slot ([L] when the capacity is not known), tree [2L], total, per_max, start)"""
        L, total, pmax, start = C.c_uint32(), C.c_float(), C.c_float(), C.c_uint64()
        _check(lib().qlx_replay_per_get(self.h, None, None, C.byref(L), None, None, None))
        tree = np.zeros(2 * L.value, np.float32)
        leaves = np.zeros(L.value, np.float32)
        _check(lib().qlx_replay_per_get(self.h, _p(leaves), _p(tree), None, C.byref(total), C.byref(pmax), C.byref(start)))
        return dict(leaves=leaves[:self.capacity], tree=tree, total=np.float32(total.value), per_max=np.float32(pmax.value),
                    start=int(start.value))


class DeepQLearningModel:
    """Nature-DQN on MI355X: fp32 (the reference's arithmetic, fp32 MFMA, bit-exact against the oracle) or, with
    precision=PREC_BF16, bf16 MFMA operands with fp32 accumulation and fp32 master weights."""

    def __init__(self, seed=2, device=0, handle=None, precision=PREC_F32):
        self._owned = handle is None
        if handle is None:
            h = C.c_void_p()
            _check(lib().qlx_model_create(ARCH_BF16 if precision == PREC_BF16 else ARCH_F32, seed, device, C.byref(h)))
            handle = h.value
        self.h = handle

    def close(self):
        head = getattr(self, "_head", None)
        if head is not None:   # (a model with a live head cannot be destroyed)
            head.close()
        if getattr(self, "_owned", False) and getattr(self, "h", None):
            lib().qlx_model_destroy(self.h)
        self.h = None

    __del__ = close

    def get(self, var, which=0):
        out = np.zeros(int(np.prod(VAR_SHAPES[var])), np.float32)
        _check(lib().qlx_model_get_var(self.h, var, which, _p(out)))
        return out.reshape(VAR_SHAPES[var])

    def set(self, var, arr, which=0):
        a = np.ascontiguousarray(arr, dtype=np.float32).reshape(-1)
        _check(lib().qlx_model_set_var(self.h, var, which, _p(a)))

    def weights(self):
        return [self.get(v) for v in range(NUM_VARS)]

    def set_weights(self, ws):
        for v, w in enumerate(ws):
            self.set(v, w)

    def iterations(self):
        return int(lib().qlx_model_iterations(self.h))

    def copy_from(self, other):
        _check(lib().qlx_model_copy_weights(self.h, other.h))

    def load_tf(self, bundle_prefix):
        """Weights, Adam slots and iterations from a TF SavedModel / checkpoint bundle of the reference model."""
        _check(lib().qlx_model_load_tf(self.h, str(bundle_prefix).encode()))

    def q_values(self, states):
        x = np.ascontiguousarray(states, dtype=np.uint8)
        n = x.shape[0]
        q = np.zeros((n, ACTION_SPACE), np.float32)
        a = np.zeros(n, np.uint8)
        _check(lib().qlx_model_predict(self.h, _p(x), n, _p(q), _p(a)))
        return q, a

    def predict_action(self, state):
        """model.rs:39-42 for one state [84][84][4] (or a batch)."""
        x = np.asarray(state, dtype=np.uint8)
        single = x.ndim == 3
        _, a = self.q_values(x[None] if single else x)
        return int(a[0]) if single else a

    def batch_predict_max_future_reward(self, states):
        x = np.ascontiguousarray(states, dtype=np.uint8)
        out = np.zeros(x.shape[0], np.float32)
        _check(lib().qlx_model_batch_max_q(self.h, _p(x), x.shape[0], _p(out)))
        return out

    def train(self, states, actions, updated_q_values, want_grads=False):
        x = np.ascontiguousarray(states, dtype=np.uint8)
        a = np.ascontiguousarray(actions, dtype=np.uint8)
        y = np.ascontiguousarray(updated_q_values, dtype=np.float32)
        B = x.shape[0]
        loss = C.c_float()
        grads = np.zeros(sum(int(np.prod(s)) for s in VAR_SHAPES), np.float32) if want_grads else None
        norms = np.zeros(NUM_VARS, np.float32)
        _check(lib().qlx_model_train(self.h, _p(x), _p(a), _p(y), B, C.byref(loss), _p(grads), _p(norms)))
        if not want_grads:
            return loss.value
        out, off = [], 0
        for s in VAR_SHAPES:
            n = int(np.prod(s))
            out.append(grads[off:off + n].reshape(s))
            off += n
        return loss.value, out, norms

    def apply_gradient(self, flat_grads, scale=1.0):
        """the update tail alone (qlx_model_apply_gradient): clip_by_norm(flat_grads * scale) + Adam; the clip norms"""
        g = np.ascontiguousarray(flat_grads, dtype=np.float32)
        assert g.size == sum(int(np.prod(s)) for s in VAR_SHAPES)
        norms = np.zeros(NUM_VARS, np.float32)
        _check(lib().qlx_model_apply_gradient(self.h, _p(g), C.c_float(scale), _p(norms)))
        return norms

    def write_checkpoint(self, path):
        _check(lib().qlx_model_write_checkpoint(self.h, path.encode()))
        return path

    def read_checkpoint(self, path):
        _check(lib().qlx_model_read_checkpoint(self.h, path.encode()))


class WideHead:
    """qlx_head: a dense layer 512 -> width (1..HEAD_MAX_WIDTH) on a4 of one fp32 DeepQLearningModel, beside its own
    512 -> 3 head.  Variables: 0 = Wh [512, width], 1 = bh [width]; which 0 weights, 1 Adam m, 2 Adam v.
    The forward, backward and gradient calls take device pointers (qlx_torch.TorchQNet drives them); the model's
    step_dev steps the head too after a backward through it.  Closed with its model (or before it)."""

    def __init__(self, model, width, seed=0):
        h = C.c_void_p()
        _check(lib().qlx_head_create(model.h, width, seed, C.byref(h)))
        self.h = h.value
        self.model = model
        self.width = int(width)
        model._head = self

    def close(self):
        if getattr(self, "h", None):
            lib().qlx_head_destroy(self.h)
            if getattr(self.model, "_head", None) is self:
                self.model._head = None
        self.h = None

    __del__ = close

    def _shape(self, var):
        return (HEAD_IN, self.width) if var == 0 else (self.width,)

    def get(self, var, which=0):
        out = np.zeros(self._shape(var) if var in (0, 1) else 1, np.float32)
        _check(lib().qlx_head_get_var(self.h, var, which, _p(out)))
        return out

    def set(self, var, arr, which=0):
        a = np.ascontiguousarray(arr, dtype=np.float32)
        if var in (0, 1) and a.size != int(np.prod(self._shape(var))):
            raise ValueError(f"variable {var} of a width-{self.width} head has shape {self._shape(var)}")
        _check(lib().qlx_head_set_var(self.h, var, which, _p(a)))

    def iterations(self):
        return int(lib().qlx_head_iterations(self.h))

    def forward_dev(self, src, n, d_z, d_q=None):
        _check(lib().qlx_head_forward_dev(self.h, C.byref(src), n, d_z, d_q))

    def backward_dev(self, src, d_dz, d_dq, batch, ticket=0):
        _check(lib().qlx_head_backward_dev(self.h, C.byref(src), d_dz, d_dq, batch, ticket))

    def grads_dev(self):
        """(device pointer, count) of the head's flat gradient buffer: Wh [512, width], then bh [width]"""
        ptr, n = C.c_void_p(), C.c_uint64()
        _check(lib().qlx_head_grads_dev(self.h, C.byref(ptr), C.byref(n)))
        return ptr.value, n.value

    def copy_weights_dev(self, other):
        _check(lib().qlx_head_copy_weights_dev(self.h, other.h))

    def values_dev(self, dist, d_z, n, d_q=None, d_actions=None, d_max_q=None):
        _check(lib().qlx_head_values_dev(self.h, C.byref(dist), d_z, n, d_q, d_actions, d_max_q))

    def dist_loss_dev(self, dist, d_z, batch_in, batch, d_dz, d_loss=None, d_sample_loss=None, d_a_star_out=None):
        _check(lib().qlx_head_dist_loss_dev(self.h, C.byref(dist), d_z, C.byref(batch_in), batch, d_dz, d_loss, d_sample_loss,
                                            d_a_star_out))

    def dist_train_dev(self, dist, src, batch_in, batch, d_z_work, d_dz_work, d_loss=None, d_sample_loss=None):
        _check(lib().qlx_head_dist_train_dev(self.h, C.byref(dist), C.byref(src), C.byref(batch_in), batch, d_z_work, d_dz_work,
                                             d_loss, d_sample_loss))

    def select_dev(self, dist, d_z, n, epsilon, seed, step, d_actions, d_max_q=None, d_q=None):
        """epsilon-greedy actions of n rows d_z [n][3 atoms] in one launch; row r draws from stream (seed, r, step, P_ACT_DEV)"""
        _check(lib().qlx_head_select_dev(self.h, C.byref(dist), d_z, n, epsilon, seed, step, d_actions, d_max_q, d_q))

    def act_dev(self, dist, src, n, epsilon, seed, step, d_actions, d_z_work, d_max_q=None, d_q=None):
        """forward_dev into d_z_work [n][3 atoms], then select_dev on it, in one call"""
        _check(lib().qlx_head_act_dev(self.h, C.byref(dist), C.byref(src), n, epsilon, seed, step, d_actions, d_max_q, d_q,
                                      d_z_work))

    def write_checkpoint(self, path):
        """Wh, bh, their Adam slots and the head's iterations in one file (the model's own file does not hold them)"""
        _check(lib().qlx_head_write_checkpoint(self.h, path.encode()))
        return path

    def read_checkpoint(self, path):
        _check(lib().qlx_head_read_checkpoint(self.h, path.encode()))


class Evaluator:
    """Policy evaluation on the GPU (qlx_evaluator, beyond the reference): n_envs fresh Breakout envs play
    episodes_per_env episodes each with a model's current weights, greedily (epsilon 0) or at a fixed epsilon; the
    Q-net forward runs over the envs still playing only (DESIGN.md "Policy evaluation")."""

    def __init__(self, n_envs, episodes_per_env=1, max_steps_per_episode=10_000, epsilon=0.0, env_seed=0x51A5EED,
                 policy_seed=1, poll_steps=0, device=0, flags=0):
        self.h = None
        self.config = _eval_config(n_envs, episodes_per_env, max_steps_per_episode, epsilon, env_seed, policy_seed,
                                   poll_steps, flags)
        h = C.c_void_p()
        _check(lib().qlx_evaluator_create(C.byref(self.config), device, C.byref(h)))
        self.h = h.value
        self.environment = BreakoutEnvironment(handle=lib().qlx_evaluator_env(self.h))

    def close(self):
        if getattr(self, "h", None):
            lib().qlx_evaluator_destroy(self.h)
        self.h = None

    __del__ = close

    def run(self, model):
        """K episodes per env with `model`'s current weights (not modified); the summary as a dict"""
        s = EvalSummary()
        _check(lib().qlx_evaluator_run(self.h, model.h, C.byref(s)))
        return _eval_summary(s)

    def run_head(self, head, dist):
        """run() with the policy of a WideHead read as `dist` (a Dist): the argmax of the head's values in place of the
        built-in Q; everything else, episodes() included, as run()"""
        s = EvalSummary()
        _check(lib().qlx_evaluator_run_head(self.h, head.h, C.byref(dist), C.byref(s)))
        return _eval_summary(s)

    def episodes(self):
        """records of the last run, each [n_envs][K]: returns, lengths, terminals (ended by done), max_q_sums"""
        shape = (self.config.n_envs, self.config.episodes_per_env)
        ret, length = np.zeros(shape, np.float32), np.zeros(shape, np.uint32)
        term, qs = np.zeros(shape, np.uint8), np.zeros(shape, np.float32)
        _check(lib().qlx_evaluator_episodes(self.h, _p(ret), _p(length), _p(term), _p(qs)))
        return dict(returns=ret, lengths=length, terminals=term.astype(bool), max_q_sums=qs)


class SelfDrivingQLearner(_LearningStats, _Metrics):
    """SelfDrivingQLearner with n parallel envs on one GPU (vector-step generalisation)."""
    _n_actions = 3

    def __init__(self, param, device=0, handle=None):
        self.param = param
        if handle is None:
            h = C.c_void_p()
            _check(lib().qlx_learner_create(C.byref(param), device, C.byref(h)))
            handle = h.value
        self.h = handle
        self.environment = BreakoutEnvironment(handle=lib().qlx_learner_env(self.h))
        self.replay_buffer = ReplayBuffer(0, 0, handle=lib().qlx_learner_replay(self.h))
        self.model = DeepQLearningModel(handle=lib().qlx_learner_model(self.h, 0))
        self.stabilized_model = DeepQLearningModel(handle=lib().qlx_learner_model(self.h, 1))

    def close(self):
        if getattr(self, "h", None):
            lib().qlx_learner_destroy(self.h)
        self.h = None

    __del__ = close

    def save(self, path):
        """Snapshot of the whole learner between vector steps (qlx_learner_save): a learner loaded from it continues
        bit for bit like this one.  Written to path + ".tmp" and renamed; QLX_SNAPSHOT_PACK=0 stores the frames raw."""
        _check(lib().qlx_learner_save(self.h, os.fspath(path).encode()))

    @classmethod
    def load(cls, path, device=0):
        """the learner a snapshot file holds (qlx_learner_load); its Parameter comes from the file"""
        param = snapshot_info(path)["params"]
        h = C.c_void_p()
        _check(lib().qlx_learner_load(os.fspath(path).encode(), device, C.byref(h)))
        return cls(param, handle=h.value)

    def vector_step(self):
        _check(lib().qlx_learner_vector_step(self.h))

    def run(self, n):
        _check(lib().qlx_learner_run(self.h, n))

    def prefill(self, n):
        """n vector steps without updates (replay fill before a measurement / parity check)"""
        _check(lib().qlx_learner_prefill(self.h, n))

    def end_episodes(self, mask):
        """end the current episode of every env with mask[e] (the max_steps_per_episode path; no transition added)"""
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        assert m.shape == (self.param.n_envs,)
        _check(lib().qlx_learner_end_episodes(self.h, _p(m)))

    def learn_till_mastered(self, max_vector_steps):
        n = C.c_uint64()
        _check(lib().qlx_learner_learn_till_mastered(self.h, max_vector_steps, C.byref(n)))
        return n.value

    def stats_events(self):
        return int(lib().qlx_learner_stats_events(self.h))

    def last_log(self):
        return _text(lib().qlx_learner_last_log, self.h)

    def sync(self):
        _check(lib().qlx_learner_sync(self.h))

    def stats(self):
        s = LearnerStats()
        _check(lib().qlx_learner_stats_get(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in LearnerStats._fields_}

    def solved(self):
        return bool(self.stats()["solved"])

    def last(self, max_updates=4096):
        N, B = self.param.n_envs, self.param.batch_size
        a = np.zeros(N, np.uint8)
        r = np.zeros(N, np.float32)
        d = np.zeros(N, np.uint8)
        losses = np.zeros(max_updates, np.float32)
        idx = np.zeros(max_updates * B, np.uint64)
        tg = np.zeros(max_updates * B, np.float32)
        nu = C.c_uint32()
        _check(lib().qlx_learner_last(self.h, _p(a), _p(r), _p(d), _p(losses), _p(idx), _p(tg), C.byref(nu)))
        n = nu.value
        return dict(actions=a, rewards=r, dones=d, losses=losses[:n], indices=idx[:n * B].reshape(n, B),
                    targets=tg[:n * B].reshape(n, B))

    def priorities(self, max_updates=4096):
        """Prioritized replay (flags & PER): IS weights [n_updates][B] of the last vector step, sum-tree leaves
        [history_buffer_len], the priority new transitions enter with."""
        B = self.param.batch_size
        w = np.zeros(max_updates * B, np.float32)
        leaves = np.zeros(self.param.history_buffer_len, np.float32)
        pmax = C.c_float()
        n = self.last()["losses"].shape[0]
        _check(lib().qlx_learner_priorities(self.h, _p(w), _p(leaves), C.byref(pmax)))
        return w[:n * B].reshape(n, B), leaves, pmax.value

    def frame_sparsity(self):
        """Fractions of the fp32 conv work the exact zero skips leave out in the last vector step (diagnostic):
        {"train": [...], "act": [...]}, each [conv1 fwd zero steps, conv1 wgrad zero steps, conv2 bg rows, conv3 bg rows]
        (train: the step's sampled states, NaN without an update; act: the current acting frames - the observations the
        next vector step acts on, after this step's env step and resets)."""
        out = np.zeros(8, np.float64)
        _check(lib().qlx_learner_frame_sparsity(self.h, _p(out)))
        return {"train": out[:4].tolist(), "act": out[4:].tolist()}

    def evaluate(self, **cfg):
        """Policy evaluation of the online model between vector steps (Evaluator's arguments but `device`); the
        learner's env, replay, counters and draws are untouched"""
        c = _eval_config(**cfg)
        s = EvalSummary()
        _check(lib().qlx_learner_evaluate(self.h, C.byref(c), C.byref(s)))
        return _eval_summary(s)

    def dist_init(self, world, rank, uid):
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(uid))
        _check(lib().qlx_learner_dist_init(self.h, world, rank, buf))

    def comm_size(self):
        """ranks of the RCCL communicator (ncclCommCount), 1 without dist_init"""
        n = C.c_int32()
        _check(lib().qlx_learner_comm_size(self.h, C.byref(n)))
        return n.value

    def profile(self, enable=True):
        _check(lib().qlx_learner_profile(self.h, 1 if enable else 0))

    def profile_filter(self, name=None, stride=1):
        """Record only scope `name` (None = all), every `stride`-th launch of it."""
        _check(lib().qlx_learner_profile_sample(self.h, None if name is None else name.encode(), stride))

    def profile_get(self, name):
        """(total_us, total_work, launches) of a profiler scope since profile() was enabled."""
        us = C.c_double()
        work = C.c_double()
        n = C.c_uint64()
        _check(lib().qlx_learner_profile_get(self.h, name.encode(), C.byref(us), C.byref(work), C.byref(n)))
        return us.value, work.value, n.value

    def profile_names(self):
        buf = C.create_string_buffer(8192)
        _check(lib().qlx_learner_profile_names(self.h, buf, 8192))
        return [n for n in buf.value.decode().split(",") if n]


def dist_unique_id():
    buf = (C.c_uint8 * 128)()
    _check(lib().qlx_dist_unique_id(buf))
    return bytes(buf)


# ---------------- BallGame (the reference's second environment / model pair) ----------------
BG_ACTION_SPACE = 5
BG_VAR_SHAPES = [(2, 2, 4, 32), (32,), (1, 1, 32, 32), (32,), (288, 512), (512,), (512, 5), (5,)]
BG_STATE_DTYPE = np.dtype([("field", "u1", (9,)), ("ball_x", "u1"), ("ball_y", "u1"), ("pad", "u1"), ("steps", "<u4"),
                           ("reset_count", "<u4")])


class BallGameEnvironment:
    """Batched `impl Environment for BallGameTestEnvironment` (ballgame_test_environment.rs:59-89)."""

    ACTION_SPACE = BG_ACTION_SPACE

    def __init__(self, n_envs=1, seed=0xBA11, device=0, handle=None):
        self._owned = handle is None
        if handle is None:
            h = C.c_void_p()
            _check(lib().qlx_bg_env_create(n_envs, seed, device, C.byref(h)))
            handle = h.value
        self.h = handle
        self.n = n_envs

    def close(self):
        if getattr(self, "_owned", False) and getattr(self, "h", None):
            lib().qlx_bg_env_destroy(self.h)
        self.h = None

    __del__ = close

    def reset(self, mask=None):
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        _check(lib().qlx_bg_env_reset(self.h, _p(m)))

    def step(self, actions):
        a = np.ascontiguousarray(actions, dtype=np.uint8)
        r = np.zeros(self.n, np.float32)
        d = np.zeros(self.n, np.uint8)
        _check(lib().qlx_bg_env_step(self.h, _p(a), _p(r), _p(d)))
        return r, d.astype(bool)

    def state(self):
        out = np.zeros((self.n, 3, 3, 4), np.uint8)
        _check(lib().qlx_bg_env_obs(self.h, _p(out)))
        return out

    def states(self):
        out = np.zeros(self.n, dtype=BG_STATE_DTYPE)
        _check(lib().qlx_bg_env_states(self.h, _p(out)))
        return out

    def set_states(self, st):
        a = np.ascontiguousarray(st, dtype=BG_STATE_DTYPE)
        assert a.shape == (self.n,)
        _check(lib().qlx_bg_env_set_states(self.h, _p(a)))

    @staticmethod
    def episode_reward_goal_mean():
        return float(lib().qlx_env_reward_goal_mean(2))


class BallGameModel:
    """The 3x3x4 -> 5 Q-model (create_ql_model_ballgame_3x3x4_5_512.py) in fp32 HIP kernels."""

    def __init__(self, seed=2, device=0, handle=None):
        self._owned = handle is None
        if handle is None:
            h = C.c_void_p()
            _check(lib().qlx_bg_model_create(seed, device, C.byref(h)))
            handle = h.value
        self.h = handle

    def close(self):
        if getattr(self, "_owned", False) and getattr(self, "h", None):
            lib().qlx_bg_model_destroy(self.h)
        self.h = None

    __del__ = close

    def get(self, var, which=0):
        out = np.zeros(int(np.prod(BG_VAR_SHAPES[var])), np.float32)
        _check(lib().qlx_bg_model_get_var(self.h, var, which, _p(out)))
        return out.reshape(BG_VAR_SHAPES[var])

    def set(self, var, arr, which=0):
        a = np.ascontiguousarray(arr, dtype=np.float32).reshape(-1)
        _check(lib().qlx_bg_model_set_var(self.h, var, which, _p(a)))

    def weights(self):
        return [self.get(v) for v in range(8)]

    def iterations(self):
        return int(lib().qlx_bg_model_iterations(self.h))

    def load_tf(self, bundle_prefix):
        """Weights, Adam slots and iterations from the reference's SavedModel variables bundle."""
        _check(lib().qlx_bg_model_load_tf(self.h, str(bundle_prefix).encode()))

    def q_values(self, states):
        x = np.ascontiguousarray(states, dtype=np.uint8)
        n = x.shape[0]
        q = np.zeros((n, BG_ACTION_SPACE), np.float32)
        a = np.zeros(n, np.uint8)
        _check(lib().qlx_bg_model_predict(self.h, _p(x), n, _p(q), _p(a)))
        return q, a

    def batch_predict_max_future_reward(self, states):
        x = np.ascontiguousarray(states, dtype=np.uint8)
        out = np.zeros(x.shape[0], np.float32)
        _check(lib().qlx_bg_model_batch_max_q(self.h, _p(x), x.shape[0], _p(out)))
        return out

    def train(self, states, actions, updated_q_values, want_grads=False):
        x = np.ascontiguousarray(states, dtype=np.uint8)
        a = np.ascontiguousarray(actions, dtype=np.uint8)
        y = np.ascontiguousarray(updated_q_values, dtype=np.float32)
        loss = np.zeros(1, np.float32)
        nrm = np.zeros(8, np.float32)
        g = np.zeros(sum(int(np.prod(s)) for s in BG_VAR_SHAPES), np.float32) if want_grads else None
        _check(lib().qlx_bg_model_train(self.h, _p(x), _p(a), _p(y), x.shape[0], _p(loss), _p(g), _p(nrm)))
        return (float(loss[0]), g, nrm) if want_grads else float(loss[0])


class BallGameLearner(_LearningStats, _Metrics):
    """SelfDrivingQLearner over n BallGame envs on one GPU (same vector-step semantics as SelfDrivingQLearner)."""
    _prefix = "qlx_bg_learner"
    _n_actions = 5

    def __init__(self, param, device=0):
        self.param = param
        h = C.c_void_p()
        _check(lib().qlx_bg_learner_create(C.byref(param), device, C.byref(h)))
        self.h = h.value
        self.environment = BallGameEnvironment(handle=lib().qlx_bg_learner_env(self.h), n_envs=param.n_envs)
        self.model = BallGameModel(handle=lib().qlx_bg_learner_model(self.h, 0))
        self.stabilized_model = BallGameModel(handle=lib().qlx_bg_learner_model(self.h, 1))

    def close(self):
        if getattr(self, "h", None):
            lib().qlx_bg_learner_destroy(self.h)
        self.h = None

    __del__ = close

    def vector_step(self):
        _check(lib().qlx_bg_learner_run(self.h, 1))

    def run(self, n):
        _check(lib().qlx_bg_learner_run(self.h, n))

    def sync(self):
        _check(lib().qlx_bg_learner_sync(self.h))

    def stats(self):
        s = LearnerStats()
        _check(lib().qlx_bg_learner_stats_get(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in LearnerStats._fields_}

    def solved(self):
        return bool(self.stats()["solved"])

    def priorities(self, max_updates=4096):
        """Prioritized replay (flags & PER): IS weights [n_updates][B] of the last vector step, sum-tree leaves, per_max."""
        B = self.param.batch_size
        w = np.zeros(max_updates * B, np.float32)
        leaves = np.zeros(self.param.history_buffer_len, np.float32)
        pmax = C.c_float()
        n = self.last()["losses"].shape[0]
        _check(lib().qlx_bg_learner_priorities(self.h, _p(w), _p(leaves), C.byref(pmax)))
        return w[:n * B].reshape(n, B), leaves, pmax.value

    def last(self, max_updates=4096):
        N, B = self.param.n_envs, self.param.batch_size
        a, r, d = np.zeros(N, np.uint8), np.zeros(N, np.float32), np.zeros(N, np.uint8)
        losses = np.zeros(max_updates, np.float32)
        idx = np.zeros(max_updates * B, np.uint64)
        tg = np.zeros(max_updates * B, np.float32)
        nu = C.c_uint32()
        _check(lib().qlx_bg_learner_last(self.h, _p(a), _p(r), _p(d), _p(losses), _p(idx), _p(tg), C.byref(nu)))
        n = nu.value
        return dict(actions=a, rewards=r, dones=d, losses=losses[:n], indices=idx[:n * B].reshape(n, B),
                    targets=tg[:n * B].reshape(n, B))


TF_DTYPES = {1: np.float32, 2: np.float64, 3: np.int32, 9: np.int64}


class SumTree:
    """Proportional prioritized-replay sum tree in HBM (per.hip; beyond the reference)."""

    def __init__(self, capacity, device=0):
        self.capacity = int(capacity)
        h = C.c_void_p()
        _check(lib().qlx_sumtree_create(self.capacity, device, C.byref(h)))
        self.h = h.value

    def close(self):
        if getattr(self, "h", None):
            lib().qlx_sumtree_destroy(self.h)
        self.h = None

    __del__ = close

    def set_leaves(self, leaves):
        x = np.ascontiguousarray(leaves, dtype=np.float32)
        if x.shape != (self.capacity,):
            raise ValueError("leaves must have shape (capacity,)")
        _check(lib().qlx_sumtree_set_leaves(self.h, _p(x)))

    def get(self):
        leaves = np.zeros(self.capacity, np.float32)
        total, pmax = C.c_float(), C.c_float()
        _check(lib().qlx_sumtree_get(self.h, _p(leaves), C.byref(total), C.byref(pmax)))
        return leaves, total.value, pmax.value

    def sample(self, seed, first_update, n_updates, rank, length, beta, batch):
        slots = np.zeros(n_updates * batch, np.uint64)
        w = np.zeros(n_updates * batch, np.float32)
        _check(lib().qlx_sumtree_sample(self.h, seed, first_update, n_updates, rank, length, beta, batch, _p(slots), _p(w)))
        return slots.reshape(n_updates, batch), w.reshape(n_updates, batch)

    def update(self, slots, td_abs, alpha, eps):
        s_ = np.ascontiguousarray(slots, dtype=np.uint64).ravel()
        t_ = np.ascontiguousarray(td_abs, dtype=np.float32).ravel()
        if s_.shape != t_.shape:
            raise ValueError("slots and td_abs must have the same length")
        _check(lib().qlx_sumtree_update(self.h, _p(s_), _p(t_), s_.shape[0], alpha, eps))


class TfBundle:
    """TF tensor bundle (variables.index + variables.data-*) read by libqlx's host-side SSTable reader."""

    def __init__(self, prefix):
        h = C.c_void_p()
        _check(lib().qlx_tf_bundle_open(str(prefix).encode(), C.byref(h)))
        self.h = h.value

    def close(self):
        if getattr(self, "h", None):
            lib().qlx_tf_bundle_close(self.h)
        self.h = None

    __del__ = close

    def entries(self):
        """{name: (dtype enum, shape tuple, byte size)}"""
        out = {}
        for i in range(lib().qlx_tf_bundle_count(self.h)):
            name = C.create_string_buffer(512)
            dt, nd, nb = C.c_int32(), C.c_int32(), C.c_int64()
            dims = np.zeros(8, np.int64)
            _check(lib().qlx_tf_bundle_entry(self.h, i, name, 512, C.byref(dt), _p(dims), C.byref(nd), C.byref(nb)))
            out[name.value.decode()] = (dt.value, tuple(int(d) for d in dims[:nd.value]), nb.value)
        return out

    def read(self, name):
        dt, shape, nbytes = self.entries()[name]
        buf = np.zeros(nbytes, np.uint8)
        _check(lib().qlx_tf_bundle_read(self.h, name.encode(), _p(buf), nbytes))
        return buf.view(TF_DTYPES[dt]).reshape(shape)
