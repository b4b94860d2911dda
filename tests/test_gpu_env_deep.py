"""GPU parity of the Breakout step kernel where a competent policy takes it, and where no play does.

The random-action parity run of test_gpu_env_replay.py almost never lets the panel meet the ball.  Here the kernel
is driven by the tape of a policy that tracks the ball (all walls, panel contacts, both bisection directions, both
bounded loops running out, the fault word, a cleared board), and by a table of directed start states, one per
branch that no play reaches (breakout_directed.py).  The bar is the CPU oracle, bit for bit; the oracle's branch
census is asserted first, so a tape or a row that stops reaching its branch fails instead of testing less.
"""
import numpy as np
import pytest

import breakout_directed as D
import oracle as O

pytestmark = pytest.mark.gpu


def _qlx():
    import qlx
    return qlx


def _play(env, tape, check, rows=None):
    """env.step(tape[t]) with a masked reset on done, nothing else: rewards, dones, and the mechanics and hashes
    after every `check` steps (before the reset of a done step, as the oracle's checkpoints)."""
    T, n = tape.shape
    rewards, dones = np.zeros((T, n), np.float32), np.zeros((T, n), bool)
    ck_states, ck_hashes = [], []
    for t in range(T):
        _, rewards[t], dones[t] = env.step(tape[t])
        if (t + 1) % check == 0:
            ck_states.append(env.mechanics())
            ck_hashes.append(env.hashes())
        if dones[t].any():
            env.reset(dones[t].astype(np.uint8))
    return rewards, dones, np.array(ck_states), np.array(ck_hashes)


def _first_step_difference(got, ref, cols=None):
    bad = np.argwhere(got != ref) if cols is None else np.argwhere((got != ref)[:, cols])
    return None if not len(bad) else tuple(int(v) for v in bad[0])


def test_tracker_tape_bit_exact_vs_oracle():
    tape, ref = D.tape_reference()
    D.assert_tape_census(ref["census"])   # a condition of the test: the tape reaches what it is here for
    assert not D.nonfinite(ref["ck_states"].ravel()).any() and not D.nonfinite(ref["states"]).any()

    env = _qlx().BreakoutEnvironment(n_envs=D.TAPE_ENVS, seed=D.TAPE_SEED)
    rewards, dones, ck_states, ck_hashes = _play(env, tape, D.TAPE_CHECK)

    for c in range(ck_states.shape[0]):
        diff = D.first_difference(ck_states[c], ref["ck_states"][c])
        assert diff is None, (f"checkpoint {c} (after step {(c + 1) * D.TAPE_CHECK}): env {diff[0]} field {diff[1]}: "
                              f"{diff[2]!r} vs oracle {diff[3]!r}")
        bad = np.flatnonzero(ck_hashes[c] != ref["ck_hashes"][c])
        assert not len(bad), f"checkpoint {c}: running checksum of env {bad[0]} differs (a step since the last one)"
    assert _first_step_difference(rewards, ref["rewards"]) is None, "(step, env) of the first reward that differs"
    assert _first_step_difference(dones, ref["dones"]) is None, "(step, env) of the first done that differs"
    assert D.first_difference(env.mechanics(), ref["states"]) is None
    assert np.array_equal(env.hashes(), ref["hashes"])
    assert np.array_equal(env.state(), ref["tensors"])


@pytest.mark.parametrize("action", [0, 1, 2])
def test_directed_states_one_tick(action):
    """set_mechanics, one step, against O.Env.set_state(...).step(action): state, reward, done, the written frame."""
    n = len(D.ROWS)
    want = [D.oracle_tick(D.STATES[i], action, env_id=i) for i in range(n)]
    for i, w in enumerate(want):   # each row still stands for its census entry
        assert w[4][D.ENTRIES[i]] > 0, (D.NAMES[i], D.ENTRIES[i])
    skipped = [i for i, w in enumerate(want) if D.nonfinite(w[0])[0]]
    assert len(skipped) < n / 4

    env = _qlx().BreakoutEnvironment(n_envs=n, seed=D.TAPE_SEED)
    env.set_mechanics(D.STATES)
    obs, rewards, dones = env.step(action)
    got = env.mechanics()
    for i, (st, r, d, frame, _) in enumerate(want):
        diff = D.first_difference(got[i:i + 1], st)
        assert diff is None, f"row {i} ({D.NAMES[i]}): field {diff[1]}: {diff[2]!r} vs oracle {diff[3]!r}"
        assert rewards[i] == r and dones[i] == d, (i, D.NAMES[i])
        if np.isfinite(st["ball_x"]) and np.isfinite(st["ball_y"]):
            slot = int(D.STATES[i]["next_slot"])
            assert np.array_equal(obs[i, :, :, slot].T, frame), f"row {i} ({D.NAMES[i]}): frame differs"


def test_directed_states_200_ticks():
    """Every row in one batch, 200 ticks of the tracker's tape from those starts, mechanics every 20 ticks."""
    n, T, K = len(D.ROWS), 200, 20
    tape = O.envs_tracker_tape(D.TAPE_SEED, n, T, start=D.STATES)
    ref = O.envs_run_tape(D.TAPE_SEED, tape, K, start=D.STATES)
    keep = ref["census"]["nonfinite"] == 0   # rows that go non-finite in the oracle are left out
    assert n - keep.sum() < n / 4, f"{n - keep.sum()} of {n} rows go non-finite"
    cols = np.flatnonzero(keep)

    env = _qlx().BreakoutEnvironment(n_envs=n, seed=D.TAPE_SEED)
    env.set_mechanics(D.STATES)
    rewards, dones, ck_states, _ = _play(env, tape, K)
    for c in range(T // K):
        diff = D.first_difference(ck_states[c][cols], ref["ck_states"][c][cols])
        assert diff is None, (f"tick {(c + 1) * K}: row {cols[diff[0]]} ({D.NAMES[cols[diff[0]]]}) field {diff[1]}: "
                              f"{diff[2]!r} vs oracle {diff[3]!r}")
    assert _first_step_difference(rewards, ref["rewards"], cols) is None
    assert _first_step_difference(dones, ref["dones"], cols) is None
    assert np.array_equal(env.state()[cols], ref["tensors"][cols])


def test_set_mechanics():
    qlx = _qlx()
    n = len(D.ROWS)
    env = qlx.BreakoutEnvironment(n_envs=n, seed=D.TAPE_SEED)
    for a in (1, 2, 0):
        env.step(a)
    obs, hashes = env.state(), env.hashes()
    assert obs.any() and hashes.all() and (env.episode_steps() == 3).all()

    env.set_mechanics(D.STATES)
    got = env.mechanics()
    assert got.tobytes() == D.STATES.tobytes(), "round trip through mechanics(): every byte, NaN payloads included"
    assert (env.episode_steps() == 0).all()
    assert np.array_equal(env.state(), obs) and np.array_equal(env.hashes(), hashes)

    env.step(0)
    assert (env.episode_steps() == 1).all()
    before = env.mechanics()
    for field, value in (("finished", 2), ("next_slot", 4), ("bricks", 1 << 60)):
        bad = D.STATES.copy()
        bad[field][n - 1] = value
        with pytest.raises(qlx.QlError):
            env.set_mechanics(bad)
        assert env.mechanics().tobytes() == before.tobytes(), f"{field}: refused, yet something was written"
        assert (env.episode_steps() == 1).all()
    ok = D.STATES.copy()
    ok["finished"][0], ok["next_slot"][1], ok["bricks"][2] = 1, 3, (1 << 60) - 1
    env.set_mechanics(ok)
    assert env.mechanics().tobytes() == ok.tobytes()
