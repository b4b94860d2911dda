"""Directed start states for the Breakout physics tick: one row per branch that play rarely or never reaches.

Each row is (name, census entry it exists for, state).  The census entry is asserted on the oracle by the tests
that use the table (CPU: test_oracle_env_deep.py, GPU: test_gpu_env_deep.py), so a row that stops reaching its
branch fails there instead of silently testing something else.  The action of a tick only sets the panel speed
after the ball has moved, so the census of one tick does not depend on it.

Geometry: field 600 x 600, ball radius 10, move 4 per tick; panel 60 x 10 with its top at y = 565;
brick id = 20 * row + col at x in [30 + 27 col, 55 + 27 col], y in [35 + 27 row, 60 + 27 row].
"""
import numpy as np

import oracle as O

FULL = (1 << 60) - 1
NAN = float("nan")


def state(ball, direction, panel_min_x, speed, bricks=FULL, panel_y=(565.0, 575.0), next_slot=0, reset_count=0):
    s = np.zeros(1, dtype=O.STATE_DTYPE)[0]
    s["ball_x"], s["ball_y"] = ball
    s["dir_x"], s["dir_y"] = direction
    s["panel_min_x"], s["panel_max_x"] = panel_min_x, panel_min_x + 60.0
    s["panel_min_y"], s["panel_max_y"] = panel_y
    s["panel_speed"] = speed
    s["bricks"] = bricks
    s["score"] = 60 - bin(bricks).count("1")
    s["next_slot"] = next_slot
    s["reset_count"] = reset_count
    return s


def _only(*ids):
    m = 0
    for i in ids:
        m |= 1 << i
    return m


# (name, census entry, state).  Mirror rows reflect x about 300 (the bricks are not symmetric: the field leaves
# 30 on the left and 32 on the right, so the mirrored seam row names its own seam).
ROWS = [
    # --- centre on the panel's boundary: the degenerate branch of the contact test
    ("panel top edge, face normal", "degenerate", state((300, 561), (0, 1), 270, 0)),
    ("panel top-left corner, vertex normal", "degenerate_vertex", state((270, 561), (0, 1), 270, 0)),
    ("panel top-left corner, upper bisection", "bisect_upper", state((270, 561), (0, 1), 270, 0, next_slot=2)),
    ("panel top-right corner, vertex normal", "degenerate_vertex", state((330, 561), (0, 1), 270, 0)),
    # --- more than one kind of object in one candidate set
    ("left wall and panel", "wall_and_panel", state((12, 553), (-1, 1), 0, 0)),
    ("right wall and panel", "wall_and_panel", state((588, 553), (1, 1), 540, 0)),
    ("left and top wall", "two_walls", state((12, 12), (-1, -1), 270, 0)),
    ("right and top wall", "two_walls", state((588, 12), (1, -1), 270, 0)),
    # A set of more than two needs three objects within 0.001 of path length of each other.  The ball's diameter
    # (20) is less than every gap of the real layout that would put three objects around it (wall to brick 30,
    # ceiling to brick 35, brick hole 29 wide with one diagonal neighbour 14.1 from the centre), so no reachable
    # state has one.  The setter takes any panel, though: a panel whose bottom face lies on the ceiling makes the
    # top-left corner a three-object contact (left wall, top wall, panel), which is what the kept >= 3 averaging needs.
    ("left wall, top wall and a panel on the ceiling", "set_gt2",
     state((12, 12), (-1, -1), 0, 0, panel_y=(-10.0, 0.0))),
    ("right wall, top wall and a panel on the ceiling", "set_gt2",
     state((588, 12), (1, -1), 540, 0, panel_y=(-10.0, 0.0))),
    # --- bounded loops and the fault word
    ("panel driven into the ball from the right", "bisect_exhausted", state((262, 570), (0, 1), 270, -160)),
    ("panel driven into the ball from the left", "bisect_exhausted", state((338, 570), (0, 1), 270, 160)),
    # The number of probes made visible.  An exhausted bisection on [0, portion] ends at hi = portion / 2^65 and its
    # way is |mv| * hi, about 1e-19: added to a coordinate it vanishes, so 64 probes or 66 would give the same state.
    # The contact point is centre + dir * way with the direction as stored, though, and the stored direction need
    # not be a unit vector: one of length 2^58..2^60 turns the last halving into a step of the ball.
    ("exhausted bisection seen through a long direction, panel moving left", "bisect_exhausted",
     state((308.4006, 572.45615), (3.3888202e17, -4.6633247e17), 245.28834, -160)),
    ("exhausted bisection seen through a long direction, panel moving right", "bisect_exhausted",
     state((235.11769, 569.30446), (-7.133657e16, -1.0168125e16), 234.30655, 160)),
    ("ball centre inside the panel", "inside", state((300, 570), (0.3, -1), 270, 0)),
    ("ball centre inside the panel, mirrored", "inside", state((300, 570), (-0.3, -1), 270, 0)),
    ("ball beyond the left wall", "wall_assert", state((5, 300), (-1, -1), 270, 0)),
    ("ball beyond the right wall", "wall_assert", state((595, 300), (1, -1), 270, 0)),
    ("ball beyond the ceiling", "wall_assert", state((300, 5), (0.2, -1), 270, 0)),
    # --- non-finite results (compared as "is NaN", see the tests)
    ("straight up into the seam of bricks 0 and 1", "nonfinite", state((56, 72), (0, -1), 270, 0)),
    ("straight up into the seam of bricks 18 and 19", "nonfinite", state((542, 72), (0, -1), 270, 0)),
    # tangent to the left wall and moving straight up: the wall's way is 0 / 0, the lone candidate of the set.  A
    # lone candidate is kept whatever its path (ContactCandidates::consider filters only from the second on).
    ("lone candidate with a NaN path at the left wall", "nonfinite", state((10, 300), (0, -1), 270, 0)),
    # --- a single brick left: the clearing tick
    ("last brick 0 from below", "cleared", state((42.5, 73), (0, -1), 270, 0, bricks=_only(0))),
    ("last brick 59 from below, slanted", "cleared", state((556, 127), (0.2, -1), 270, 0, bricks=_only(59))),
    ("last brick 30 on its corner", "cleared", state((316, 99), (1, -1), 270, 0, bricks=_only(30))),
    ("last two bricks 40 and 41 at their seam", "multi_brick", state((56, 127), (0, -1), 270, 0, bricks=_only(40, 41))),
    # --- dir as init_state leaves it (not unit length)
    ("launch direction, first tick", "ticks", state((300, 300), (-0.25, -1), 270, 0)),
    # (the contact point is centre + dir * way with dir as stored: 40 times too far here, through three rows)
    ("long direction into brick 45", "moves3", state((177, 126), (3, -40), 270, 0)),
    ("long direction into the panel", "panel_contact", state((300, 553), (6, 8), 270, 0)),
    ("short direction into the left wall", "wall_left", state((12, 300), (-0.03, -0.01), 270, 0)),
    # --- panel clamps with the ball in play
    ("panel reaches the left border", "clamp_left", state((300, 300), (0.2, -1), 2, -160)),
    ("panel reaches the right border", "clamp_right", state((300, 300), (0.2, -1), 538, 160)),
    # --- the angle test: a ball leaving the panel it still touches
    ("leaving the panel upwards", "angle_reject", state((300, 558.5), (0, -1), 270, 0)),
    # --- non-finite start states: every loop of the tick is bounded, so these end like any other
    ("ball x is NaN", "nonfinite", state((NAN, 300), (0.2, -1), 270, 0)),
    ("ball y is +infinity", "nonfinite", state((300, float("inf")), (0.2, -1), 270, 0)),
    ("direction is NaN", "nonfinite", state((300, 300), (NAN, -1), 270, 0)),
    ("direction x is infinite", "nonfinite", state((300, 300), (float("inf"), -1), 270, 0)),
    # --- NaN paths in the candidate filter (the shortest path skips them, the filter drops them)
    ("NaN path at the left wall beside a finite one at the ceiling", "filter_dropped", state((10, 12), (0, -1), 270, 0)),
    # consider filters after every insertion: of three NaN paths (all walls; panel and bricks fail the angle test
    # on the way down) the second empties the set and the third stands alone, so the ball is reflected
    ("three NaN paths, the last stands alone", "wall_assert", state((NAN, NAN), (0.2, 1), 270, 0)),
]

NAMES = [r[0] for r in ROWS]
ENTRIES = [r[1] for r in ROWS]
STATES = np.array([r[2] for r in ROWS], dtype=O.STATE_DTYPE)

FLOAT_FIELDS = [k for k in O.STATE_DTYPE.names if O.STATE_DTYPE[k].kind == "f"]


def nonfinite(st):
    """Per record: any float field of the state is NaN or infinite."""
    st = np.atleast_1d(st)
    bad = np.zeros(st.shape, bool)
    for k in FLOAT_FIELDS:
        bad |= ~np.isfinite(st[k])
    return bad


def first_difference(got, ref):
    """The first (record, field) at which two state arrays differ, None if none does.  Every field compares exactly
    (as numbers: the sign of a zero is no part of the contract, as in the running checksum); where the reference
    holds a NaN the other side must hold a NaN too (neither are the sign and payload of a generated NaN)."""
    got, ref = np.atleast_1d(got), np.atleast_1d(ref)
    for i in range(ref.shape[0]):
        for k in O.STATE_DTYPE.names:
            g, r = got[k][i], ref[k][i]
            same =bool(np.isnan(g)) if k in FLOAT_FIELDS and np.isnan(r) else g == r
            if not same:
                return i, k, g, r
    return None


def oracle_tick(row_state, action, env_id=0):
    """One oracle step from a directed state: (state, reward, done, written frame [y][x], census record)."""
    env = O.Env(0x51A5EED, env_id).set_state(row_state)
    cz = env.census()
    slot = int(row_state["next_slot"])
    r, d = env.step(action)
    return env.state(), r, d, env.frame(slot), cz.copy()


# ---- the tracker tape of the deep parity test ---------------------------------------------------------------------
TAPE_SEED, TAPE_ENVS, TAPE_STEPS, TAPE_CHECK = 0x51A5EED, 61, 9000, 250

# what the tape has to reach (census entry, least count); the test asserts it before any GPU work
TAPE_REACH = [("wall_left", 1), ("wall_right", 1), ("wall_top", 1), ("panel_contact", 1), ("clamp_left", 1),
              ("clamp_right", 1), ("inside", 1), ("bisect_lower", 1), ("bisect_upper", 1), ("bisect_exhausted", 1),
              ("moves3", 1), ("moves_exhausted", 1), ("wall_assert", 1), ("filter_dropped", 1), ("multi_brick", 1),
              ("angle_reject", 1), ("cleared", 1), ("max_score", 60)]

_tape_cache = {}


def tape_reference():
    """(tape, oracle run) of the tracking policy, computed once per process and never written to."""
    if not _tape_cache:
        tape = O.envs_tracker_tape(TAPE_SEED, TAPE_ENVS, TAPE_STEPS)
        ref = O.envs_run_tape(TAPE_SEED, tape, TAPE_CHECK)
        for a in [tape] + [v for v in ref.values()]:
            a.setflags(write=False)
        _tape_cache["v"] = (tape, ref)
    return _tape_cache["v"]


def assert_tape_census(census):
    tot = O.census_total(census)
    missing = [(k, tot[k]) for k, least in TAPE_REACH if tot[k] < least]
    assert not missing, f"the tracker tape no longer reaches: {missing}"
    assert tot["nonfinite"] == 0, "an env of the tracker tape went non-finite"
