"""bench.py's contract on a small workload (256 envs, replay 20,000, B = 32): a plain run prints the headline line alone,
--steps sets the timed vector steps, --dump-outputs writes the last timed step's outputs as float32 / float64 .npy files
that are identical from run to run, and --full adds the event-timed figures without changing what is computed.

The benchmark is started three times, once per module (plain, plain again, --full with the runs beside the headline and
the CPU baseline switched off); every test reads those results."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP, ENVS, BATCH, REPLAY = 10, 1, 256, 32, 20_000
SMALL = ["--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP), "--envs", str(ENVS), "--batch", str(BATCH),
         "--replay", str(REPLAY)]
NO_BESIDE = ["--beside-steps", "0", "--nomemo-steps", "0", "--dense-steps", "0", "--refwork-steps", "0", "--dp1-steps", "0",
             "--c5-steps", "0", "--cpu-sample", "0"]
HEADLINE_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"}
FULL_ONLY_KEYS = {"roofline", "mfma_per_layer", "replay_sampling", "clip_adam", "components_event_timed", "skipped_fractions"}
BESIDE_KEYS = {"no_target_memo", "dense_frames", "reference_work", "dp_single_rank", "c5_shard", "bf16_beside", "cpu_baseline"}


def _bench(extra, dump):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + extra + ["--dump-outputs", str(dump)],
                         capture_output=True, text=True, env=env, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout   # ONE JSON line on stdout
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(dump, f)) for f in sorted(os.listdir(dump))}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bench")
    return {"plain": _bench([], d / "a"), "again": _bench([], d / "b"), "full": _bench(["--full"] + NO_BESIDE, d / "f")}


def test_plain_run_prints_the_headline_only(runs):
    line, _ = runs["plain"]
    assert HEADLINE_KEYS <= set(line)
    assert not (FULL_ONLY_KEYS | BESIDE_KEYS) & set(line)
    assert line["unit"] == "env-steps/s" and line["higher_is_better"] is True and line["dtype"] == "fp32"
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["n_gpus"] == 1
    # value and ms_per_step are the same measurement: ENVS env-steps per timed vector step (both rounded in the line)
    assert line["ms_per_step"] > 0
    assert abs(line["value"] * line["ms_per_step"] / 1e3 - ENVS) <= 1e-3 * ENVS


def test_steps_sets_the_timed_vector_steps(runs):
    """The learner's counters after the timed window: prefill + W + the one step of the profile pass + K vector steps,
    and every vector step of the window is in grad_updates_per_sec (ENVS / update_after_actions updates each)."""
    line, dump = runs["plain"]
    stats = dict(zip(("step_count", "vec_steps", "update_count", "episode_count", "replay_len"), dump["stats"]))
    assert stats["vec_steps"] == line["steady_state"]["prefill_vector_steps"] + WARMUP + 1 + STEPS
    assert stats["step_count"] == stats["vec_steps"] * ENVS and stats["replay_len"] == REPLAY
    ua = line["config"]["update_after_actions"]
    assert stats["update_count"] == (WARMUP + 1 + STEPS) * ENVS // ua
    # (rates are rounded to 2 decimals and ms_per_step to 3 in the line)
    assert abs(line["grad_updates_per_sec"] * line["ms_per_step"] / 1e3 - ENVS // ua) <= 2e-3 * (ENVS // ua)


def test_dump_holds_the_last_steps_outputs(runs):
    _, dump = runs["plain"]
    U = ENVS // (BATCH // 8)
    want = {"last_actions": (ENVS,), "last_rewards": (ENVS,), "last_dones": (ENVS,), "last_losses": (U,),
            "last_indices": (U, BATCH), "last_targets": (U, BATCH), "env_mechanics": (ENVS, 16),
            "acting_frames": (64, 84, 84, 4), "acting_frames_envs": (64,), "stats": (8,),
            "online_6_full_layer_kernel": (3136, 512), "online_9_action_layer_bias": (3,)}
    for k, shape in want.items():
        assert dump[k].shape == shape, k
    assert len(dump) == 10 + 10
    assert all(a.dtype in (np.float32, np.float64) for a in dump.values())
    assert sum(a.nbytes for a in dump.values()) <= 64_000_000
    assert all(np.isfinite(a).all() for a in dump.values())
    assert set(np.unique(dump["last_actions"])) <= {0.0, 1.0, 2.0}
    idx = dump["last_indices"]
    assert (idx >= 0).all() and (idx < REPLAY).all() and (idx == np.round(idx)).all()
    assert np.abs(dump["online_6_full_layer_kernel"]).max() > 0 and dump["acting_frames"].max() > 0


def test_dump_is_identical_from_run_to_run(runs):
    (_, a), (_, b) = runs["plain"], runs["again"]
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k


def test_full_adds_figures_and_computes_the_same(runs):
    (plain, a), (full, f) = runs["plain"], runs["full"]
    assert (HEADLINE_KEYS | FULL_ONLY_KEYS) <= set(full)
    # the runs beside the headline were switched off (--cpu-sample 0 leaves its key, holding null)
    assert BESIDE_KEYS & set(full) == {"cpu_baseline"} and full["cpu_baseline"] is None
    assert "act_forward" in full["components_event_timed"]
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup", "steady_state"):
        assert full[k] == plain[k], k
    assert sorted(a) == sorted(f)
    for k in a:
        assert np.array_equal(a[k], f[k]), k
