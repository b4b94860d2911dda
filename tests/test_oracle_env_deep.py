"""The oracle side of the deep Breakout env tests, on the CPU: the fault word of an exhausted bisection, the state
setter, the branch census, and the two facts the GPU tests in test_gpu_env_deep.py rest on (the tracker tape reaches
every branch it is there for; every directed row reaches its own)."""
import numpy as np
import pytest

import breakout_directed as D
import oracle as O

SEED = 0x51A5EED


def test_exhausted_bisection_sets_the_fault_word():
    """The panel driven into the ball: every probe penetrates, the bisection runs out, and the state says so."""
    for name in ("panel driven into the ball from the right", "panel driven into the ball from the left"):
        st, _, _, _, cz = D.oracle_tick(D.STATES[D.NAMES.index(name)], 0)
        assert cz["bisect_exhausted"] == 1 and cz["bisect_max_depth"] == 64
        assert st["fault"] & 4, name
    # the KAT entry point has no state to fault and keeps its result
    assert O.rect_check((262.0, 570.0), 10.0, (0.0, 4.0), (266.8, 565.0), (326.8, 575.0)) is None


def test_set_state_round_trip():
    env = O.Env(SEED, 3)
    for i, st in enumerate(D.STATES):
        got = env.set_state(st).state()
        assert D.first_difference(got, st) is None, (D.NAMES[i], D.first_difference(got, st))
    # frames are left alone
    env = O.Env(SEED, 3)
    env.step(1)
    before = env.tensor().copy()
    env.set_state(D.STATES[0])
    assert np.array_equal(env.tensor(), before)


def test_set_state_keeps_brick_order_after_removals():
    """A state reached by play and the same state put in by set_state go on identically: the brick vector's order
    is the order of the candidate sums."""
    tape = O.envs_tracker_tape(SEED, 4, 1500)
    for e in range(4):
        played = O.Env(SEED, e)
        for t in range(700):
            _, done = played.step(tape[t, e])
            if done:
                played.reset()
        st = played.state()
        assert 0 < bin(int(st["bricks"])).count("1") < 60, "no brick removed yet: the test would show nothing"
        copy = O.Env(SEED, e).set_state(st)
        for t in range(700, 1500):
            ra, da = played.step(tape[t, e])
            rb, db = copy.step(tape[t, e])
            assert (ra, da) == (rb, db) and D.first_difference(copy.state(), played.state()) is None, (e, t)
            if da:
                played.reset()
                copy.reset()
    # a mask with holes: ids come back in creation order
    mask = D.FULL & ~((1 << 0) | (1 << 21) | (1 << 59))
    st = D.STATES[0].copy()
    st["bricks"] = mask
    assert int(O.Env(SEED, 0).set_state(st).state()["bricks"]) == mask


def test_random_driver_never_meets_the_right_or_top_wall():
    """The motivation of the deep tests, kept honest: the random-action parity run reaches few branches."""
    _, h, cz = O.envs_run_census(SEED, 1024, 600, 9)
    tot = O.census_total(cz)
    assert tot["wall_right"] == 0 and tot["wall_top"] == 0
    assert tot["bisect_upper"] == 0 and tot["bisect_exhausted"] == 0 and tot["moves3"] == 0 and tot["wall_assert"] == 0
    assert tot["bisect_max_depth"] <= 2 and tot["max_score"] == 3
    assert tot["ticks"] == 1024 * 600


def test_census_does_not_change_the_run():
    st0, h0, _, _, _ = O.envs_run(SEED, 256, 400, 9, 50)
    st1, h1, cz = O.envs_run_census(SEED, 256, 400, 9, 50)
    assert np.array_equal(h0, h1) and D.first_difference(st1, st0) is None
    assert O.census_total(cz)["ticks"] == 256 * 400


def test_tracker_tape_reaches_every_branch():
    tape, ref = D.tape_reference()
    assert tape.shape == (D.TAPE_STEPS, D.TAPE_ENVS) and set(np.unique(tape)) == {0, 1, 2}
    D.assert_tape_census(ref["census"])
    # the fault word is seen at checkpoints, bits 1 and 4 both
    faults = np.bitwise_or.reduce(ref["ck_states"]["fault"].ravel())
    assert faults & 1 and faults & 4
    # the tape is the policy's: replaying it with the tracker's rule gives the same actions
    env = O.Env(D.TAPE_SEED, 60)
    for t in range(300):
        s = env.state()
        pc = np.float32((s["panel_min_x"] + s["panel_max_x"]) / np.float32(2))
        want = 1 if s["ball_x"] < pc - np.float32(10) else (2 if s["ball_x"] > pc + np.float32(10) else 0)
        assert tape[t, 60] == want, t
        if env.step(want)[1]:
            env.reset()


@pytest.mark.parametrize("i", range(len(D.ROWS)), ids=[n.replace(" ", "_") for n in D.NAMES])
def test_directed_row_reaches_its_branch(i):
    _, _, _, _, cz = D.oracle_tick(D.STATES[i], 0)
    assert cz[D.ENTRIES[i]] > 0, (D.NAMES[i], {k: int(cz[k]) for k in O.CENSUS_FIELDS if cz[k]})


def test_directed_table_shape():
    assert len(D.ROWS) >= 24 and len(set(D.NAMES)) == len(D.NAMES)
    bad = sum(bool(D.nonfinite(D.oracle_tick(st, 0)[0])[0]) for st in D.STATES)
    assert 0 < bad < len(D.ROWS) / 4
