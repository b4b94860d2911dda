"""Acting with, evaluating and checkpointing a distributional head on the GPU (include/qlx.h "acting with, evaluating and
checkpointing a distributional head"; csrc/dist_loss.hip k_dist_select, csrc/evaluator.hip, csrc/head_wide.hip).

1. qlx_head_select_dev: qlx_head_values_dev's bits at epsilon 0; with epsilon > 0 the oracle's Philox draws (purpose 9,
   c1 = row, c2 = step; the f64 from word 0, the random action from word 2) decide, max_q and q stay the greedy values.
2. qlx_head_act_dev is qlx_head_forward_dev + qlx_head_select_dev, bit for bit, with one forward ticket.
3. qlx_evaluator_run_head against the evaluator's contract (tests/test_gpu_evaluator.py's restatement over the CPU oracle's
   game and draws), the values of a row defined by qlx_head_forward_dev + qlx_head_values_dev.
4. A constant policy: the built-in head's run bit for bit, compaction, poll_steps, a categorical twin.
5. A run disturbs nothing of a model and head in training.
6. State errors launch nothing.
7. Head checkpoints continue a run bit for bit; refused files change nothing.
All comparisons are made on bytes copied back to the host."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from head_eval_helpers import (DEV, LAY, P_ACT_DEV, QT, assert_same_state, dev, full_state, head_state, host, indices,
                               make_dist, make_world, net, qlx, same, summary_lists, update)
import oracle as O
from test_gpu_evaluator import (EPSILON, GREEDY, TAIL, TAIL_LENGTHS, assert_records, check_summary, expected_steps,
                                restatement, zero_model)

pytestmark = pytest.mark.gpu

Q_ATOMS = [1, 2, 51, 64, 65, 341]   # one quantile; one wave, ragged; one full wave; a second wave; all six lane rounds
C_ATOMS = [2, 3, 51, 64, 65, 341]
ROWS = [1, 5, 100]                  # a row alone; a ragged last block of four-row blocks; 25 blocks
E_INVALID, E_STATE = -1, -4


@pytest.fixture(scope="module")
def world():
    w = make_world()
    yield w
    w[1].close()
    w[0].close()


def random_z(rng, kind, n, N):
    """seeded rows plus, where n has room, directed ones: an exact tie of the two best values (row 3), all three equal
    (row 4), and for logits +-60 (row 2)"""
    z = ((1.5 if kind == "quantile" else 3.0) * rng.normal(size=(n, 3, N))).astype(np.float32)
    if n >= 5:
        z[3, 2] = z[3, 1]
        # (action 0 below them: lower quantiles, or logits that put the mass on the lowest atoms)
        z[3, 0] = z[3, 1] - np.float32(1) if kind == "quantile" else np.linspace(30, -30, N, dtype=np.float32)
        z[4, 1] = z[4, 0]
        z[4, 2] = z[4, 0]
        if kind == "categorical":
            z[2] = np.where(rng.random((3, N)) < 0.5, np.float32(60), np.float32(-60))
    return z.reshape(n, 3 * N)


def values(T, dist, z):
    q, a, mq = (host(t) for t in T.head_values(z, dist))
    return q, a, mq


def select(T, dist, z, epsilon, seed, step):
    """the C call on a device tensor z -> host (actions, max_q, q)"""
    n = z.shape[0]
    a = torch.full((n,), 9, dtype=torch.uint8, device=DEV)
    mq = torch.empty(n, dtype=torch.float32, device=DEV)
    q = torch.empty((n, 3), dtype=torch.float32, device=DEV)
    T._run(None, None, (z, a, mq, q),
           lambda: qlx.lib().qlx_head_select_dev(T.head.h, C.byref(dist.c), z.data_ptr(), n, epsilon, seed, step, a.data_ptr(),
                                                 mq.data_ptr(), q.data_ptr()))
    return host(a), host(mq), host(q)


def expected_actions(greedy, epsilon, seed, step, rows=None):
    """(actions, random mask) by the oracle's generators; rows: the stream index of each row (default: its position)"""
    L = O.lib()
    rows = range(len(greedy)) if rows is None else rows
    rnd = np.array([epsilon > 0 and epsilon > L.orc_gen_f64_01(seed, r, step, P_ACT_DEV) for r in rows], bool)
    drawn = np.array([L.orc_gen_u8(seed, r, step, P_ACT_DEV, 2, 3) for r in rows], np.uint8)
    return np.where(rnd, drawn, greedy).astype(np.uint8), rnd


# ---------------------------------------------------------------- 1. select

@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("kind,N", [("quantile", N) for N in Q_ATOMS] + [("categorical", N) for N in C_ATOMS])
def test_select_is_values_and_the_oracle_draws(kind, N, n):
    T = net()
    T.attach_head(3 * N)
    dist = make_dist(kind, N)
    z = dev(random_z(np.random.default_rng(31 * N + n), kind, n, N))
    q, greedy, mq = values(T, dist, z)
    assert np.isfinite(q).all()
    if n >= 5:
        assert greedy[3] == 1 and q[3, 1] == q[3, 2] and greedy[4] == 0 and q[4, 0] == q[4, 1] == q[4, 2]
    seed, step = 0xAC7 + N, 1000 + n
    for epsilon in (0.0, 0.25, 1.0):
        a, got_mq, got_q = select(T, dist, z, epsilon, seed, step)
        want, rnd = expected_actions(greedy, epsilon, seed, step)
        assert same(got_q, q) and same(got_mq, mq), epsilon
        assert np.array_equal(a, want), epsilon
        if epsilon == 0.0:
            assert not rnd.any() and np.array_equal(a, greedy)
        if epsilon == 1.0:
            assert rnd.all()
        if epsilon == 0.25 and n == 100:
            assert rnd.any() and not rnd.all() and (a != greedy).any()
        again = select(T, dist, z, epsilon, seed, step)
        assert same(again[0], a) and same(again[1], got_mq) and same(again[2], got_q)
    # the optional outputs are optional
    only = T.select(z, dist, 0.25, seed, step)
    assert np.array_equal(host(only), expected_actions(greedy, 0.25, seed, step)[0])
    T.sync()
    T.close()


@pytest.mark.parametrize("kind", ["quantile", "categorical"])
def test_select_row_is_independent_of_its_batch(kind):
    """a row alone, first or last in a batch of 100: the same values; the draw belongs to the row's index"""
    N, n = 51, 100
    T = net()
    T.attach_head(3 * N)
    dist = make_dist(kind, N)
    zh = random_z(np.random.default_rng(77), kind, n, N)
    _, greedy, _ = values(T, dist, dev(zh))
    full = select(T, dist, dev(zh), 0.25, 5, 9)
    alone = select(T, dist, dev(zh[:1]), 0.25, 5, 9)
    assert all(same(x[:1], y) for x, y in zip(full, alone))
    flip = select(T, dist, dev(zh[::-1].copy()), 0.25, 5, 9)
    assert same(flip[1][::-1], full[1]) and same(flip[2][::-1], full[2])
    want, _ = expected_actions(greedy[::-1], 0.25, 5, 9)   # row r of the flipped batch draws from stream r
    assert np.array_equal(flip[0], want)
    T.sync()
    T.close()


# ---------------------------------------------------------------- 2. act

@pytest.mark.parametrize("kind", ["quantile", "categorical"])
def test_act_is_forward_then_select(world, kind):
    N = 51
    env, rb = world
    T = net()
    T.attach_head(3 * N, seed=8)
    dist = make_dist(kind, N)
    L = qlx.lib()
    for src in (dict(env=env), dict(replay=rb, indices=indices(world, 5)), dict(replay=rb, indices=indices(world, 100, 1))):
        s, n, ins = T._source(None, src.get("env"), src.get("replay"), src.get("indices"), "s", LAY)
        zw = torch.zeros((n, 3 * N), dtype=torch.float32, device=DEV)
        a = torch.full((n,), 9, dtype=torch.uint8, device=DEV)
        mq = torch.empty(n, dtype=torch.float32, device=DEV)
        q = torch.empty((n, 3), dtype=torch.float32, device=DEV)
        t0 = T.forward_ticket()
        T._run(src.get("env"), src.get("replay"), ins + (zw, a, mq, q),
               lambda: L.qlx_head_act_dev(T.head.h, C.byref(dist.c), C.byref(s), n, 0.25, 11, 3, a.data_ptr(), mq.data_ptr(),
                                          q.data_ptr(), zw.data_ptr()))
        assert T.forward_ticket() == t0 + 1
        with torch.no_grad():
            _, z = T.forward(head=True, layout=LAY, **src)
        parts = select(T, dist, z, 0.25, 11, 3)
        assert same(host(zw), host(z)) and np.abs(host(z)).max() > 0
        assert same(host(a), parts[0]) and same(host(mq), parts[1]) and same(host(q), parts[2])
    T.sync()
    T.close()


# ---------------------------------------------------------------- 3. the evaluator's contract

def run_head(cfg, T, dist, poll_steps=8):
    ev = qlx.Evaluator(poll_steps=poll_steps, **cfg)
    try:
        s = T.evaluate(ev, dist)
        return s, ev.episodes()
    finally:
        ev.close()


@pytest.fixture(scope="module")
def net7():
    T = net(seed=7, reserve=16)
    yield T
    T.close()


@pytest.mark.parametrize("case", ["greedy", "epsilon"])
@pytest.mark.parametrize("kind", ["quantile", "categorical"])
def test_run_head_is_the_evaluators_contract(net7, kind, case):
    N = 51
    T = net7
    head = T.attach_head(3 * N, seed=21)
    dist = make_dist(kind, N)
    try:
        def q_of(xs):   # the product's pinned kernels define the values of a row
            with torch.no_grad():
                _, z = T.forward(dev(np.stack(xs)), layout="nhwc_slot", head=True)
            return host(T.head_values(z, dist, want="q"))

        cfg = GREEDY if case == "greedy" else EPSILON
        rec, counts, randoms = restatement(q_of, cfg["n_envs"], cfg["episodes_per_env"], cfg["max_steps_per_episode"],
                                           cfg["epsilon"], cfg["env_seed"], cfg.get("policy_seed", 1))
        if case == "epsilon":
            assert 0.15 * counts.sum() < randoms < 0.35 * counts.sum()
        s, got = run_head(cfg, T, dist)
        assert_records(got, rec)
        check_summary(s, rec, counts, 8)
        assert np.abs(rec["max_q_sums"]).max() > 0
    finally:
        head.close()


# ---------------------------------------------------------------- 4. a constant policy and compaction

def constant_head(T, kind):
    """values exactly [1, 0, 0] (three quantiles), or logits that favour action 0 by a wide margin (three atoms on [-10, 10])"""
    head = T.attach_head(9)
    head.set(0, np.zeros((512, 9), np.float32))
    if kind == "quantile":
        head.set(1, np.float32([1] * 3 + [0] * 6))
    else:
        head.set(1, np.float32([0, 0, 40] + [40, 0, 0] * 2))
    return head


def test_constant_policy_is_the_builtin_heads_run(net7, monkeypatch):
    T = net7
    m = zero_model(0)
    head = constant_head(T, "quantile")
    dist = QT.Quantile(3)
    try:
        ev = qlx.Evaluator(poll_steps=8, **TAIL)
        try:
            ref_s, ref = ev.run(m), ev.episodes()
            s, got = T.evaluate(ev, dist), ev.episodes()   # the same evaluator serves both kinds of run
        finally:
            ev.close()
        assert ref["lengths"][:, 0].tolist() == TAIL_LENGTHS
        assert_records(got, ref)
        assert summary_lists(s) == summary_lists(ref_s)
        assert (s["vector_steps"], s["forward_samples"]) == expected_steps(ref["lengths"], 8)
        assert s["forward_samples"] < 16 * s["vector_steps"] / 4 and s["action_counts"].tolist() == [sum(TAIL_LENGTHS), 0, 0]
        for P in (1, 32):
            s, got = run_head(TAIL, T, dist, poll_steps=P)
            assert_records(got, ref)
            assert (s["vector_steps"], s["forward_samples"]) == expected_steps(ref["lengths"], P)
        monkeypatch.setenv("QLX_EVAL_COMPACT", "0")   # read once at qlx_evaluator_create
        s, got = run_head(TAIL, T, dist)
        assert_records(got, ref)
        assert (s["vector_steps"], s["forward_samples"]) == expected_steps(ref["lengths"], 8, compact=False)
        monkeypatch.delenv("QLX_EVAL_COMPACT")
        monkeypatch.setenv("QLX_EVAL_HEAD_FUSED", "0")   # values, then the built-in select: the same records
        s, got = run_head(TAIL, T, dist)
        assert_records(got, ref)
        assert summary_lists(s) == summary_lists(ref_s)
        monkeypatch.delenv("QLX_EVAL_HEAD_FUSED")
        head.close()
        head = constant_head(T, "categorical")
        s, got = run_head(TAIL, T, QT.Categorical(3, -10.0, 10.0))
        for key in ("returns", "lengths", "terminals"):
            assert same(got[key], ref[key]), key
        assert same(s["action_counts"], ref_s["action_counts"])
    finally:
        head.close()
        m.close()


# ---------------------------------------------------------------- 5. undisturbed

@pytest.mark.parametrize("kind", ["quantile", "categorical"])
def test_run_head_disturbs_nothing(world, kind):
    N = 51
    dist = make_dist(kind, N)
    nets = [net(seed=5), net(seed=5)]
    for T in nets:
        T.attach_head(3 * N, seed=8)
    cfg = dict(n_envs=24, episodes_per_env=1, max_steps_per_episode=12, epsilon=0.05, env_seed=11, policy_seed=12)
    losses = [[update(T, world, dist, 0)] for T in nets]
    before = full_state(nets[0])
    ticket = nets[0].forward_ticket()
    s, _ = run_head(cfg, nets[0], dist, poll_steps=4)
    assert s["episodes"] == 24 and s["vector_steps"] == 12 and s["env_steps"] == 24 * 12
    assert nets[0].forward_ticket() != ticket   # the run's forwards took tickets of their own
    assert_same_state(full_state(nets[0]), before)
    for k in (1, 2):
        for T, l in zip(nets, losses):
            l.append(update(T, world, dist, k))
    assert all(same(x, y) and np.isfinite(x) for x, y in zip(*losses))
    assert_same_state(full_state(nets[0]), full_state(nets[1]))
    assert nets[0].model.iterations() == 3 and nets[0].head.iterations() == 3
    for T in nets:
        T.sync()   # clean: no sticky flag
        T.close()


# ---------------------------------------------------------------- 6. state errors

def test_state_errors(world):
    L = qlx.lib()
    T = net(reserve=8)
    head = T.attach_head(153)
    z = torch.zeros((16, 153), dtype=torch.float32, device=DEV)
    zw = torch.full((16, 153), 7.0, dtype=torch.float32, device=DEV)
    a = torch.full((16,), 7, dtype=torch.uint8, device=DEV)
    obs = torch.zeros((16, 4, 84, 84), dtype=torch.uint8, device=DEV)
    s = qlx.StatesDev(obs=obs.data_ptr(), layout=qlx.OBS_NCHW_TIME)
    good, wrong = qlx.Dist(qlx.DIST_QUANTILE, 51, 0, 0), qlx.Dist(qlx.DIST_QUANTILE, 50, 0, 0)
    ev = qlx.Evaluator(n_envs=4, max_steps_per_episode=5)
    summary = qlx.EvalSummary()
    ticket = T.forward_ticket()
    torch.cuda.synchronize()
    calls = lambda d, n: (   # noqa: E731
        L.qlx_head_select_dev(head.h, C.byref(d), z.data_ptr(), n, 0.5, 1, 0, a.data_ptr(), None, None),
        L.qlx_head_act_dev(head.h, C.byref(d), C.byref(s), n, 0.5, 1, 0, a.data_ptr(), None, None, zw.data_ptr()))
    try:
        for status in calls(wrong, 4) + (L.qlx_evaluator_run_head(ev.h, head.h, C.byref(wrong), C.byref(summary)),):
            assert status == E_INVALID and b"atoms" in L.qlx_last_error()
        for status in calls(good, 16):
            assert status == E_STATE and b"reserve" in L.qlx_last_error()
        assert L.qlx_evaluator_episodes(ev.h, None, None, None, None) == E_STATE
        with pytest.raises(qlx.QlError, match="status -4"):
            ev.episodes()
        assert T.forward_ticket() == ticket
        T.sync()
        assert (host(zw) == 7).all() and (host(a) == 7).all(), "a failed call launched something"
    finally:
        ev.close()
        T.close()


# ---------------------------------------------------------------- 7. checkpoints

@pytest.mark.parametrize("kind", ["quantile", "categorical"])
def test_checkpoints_continue_bit_for_bit(world, kind, tmp_path):
    N = 51
    dist = make_dist(kind, N)
    A = net(seed=5)
    A.attach_head(3 * N, seed=8)
    for k in (0, 1):
        update(A, world, dist, k)
    mpath, hpath = str(tmp_path / "model.ckpt"), str(tmp_path / "head.ckpt")
    A.model.write_checkpoint(mpath)
    assert A.head.write_checkpoint(hpath) == hpath
    assert os.path.getsize(hpath) == 8 + 16 + 3 * 4 * 513 * 3 * N
    with open(hpath, "rb") as f:
        raw = f.read()
    assert raw[:8] == b"QLXHEAD1" and np.frombuffer(raw[8:24], "<i8").tolist() == [3 * N, 2]
    loss_a = update(A, world, dist, 2)
    B = net(seed=6)
    B.attach_head(3 * N, seed=9)
    update(B, world, dist, 7)   # other weights, other Adam slots, another iteration count
    B.model.read_checkpoint(mpath)
    B.head.read_checkpoint(hpath)
    assert B.head.iterations() == 2
    loss_b = update(B, world, dist, 2)
    assert same(loss_a, loss_b) and np.isfinite(loss_a)
    assert_same_state(full_state(A), full_state(B))
    assert A.head.iterations() == 3

    # refused files change nothing
    before = head_state(B)
    other = net(seed=5)
    other.attach_head(3 * (N + 1))
    wide = other.head.write_checkpoint(str(tmp_path / "wide.ckpt"))
    files = {"width": wide, "short": str(tmp_path / "short.ckpt"), "magic": str(tmp_path / "magic.ckpt"),
             "header": str(tmp_path / "header.ckpt")}
    with open(files["short"], "wb") as f:
        f.write(raw[:-4])
    with open(files["magic"], "wb") as f:
        f.write(b"QLXCKPT1" + raw[8:])
    with open(files["header"], "wb") as f:
        f.write(raw[:20])
    for why, path in files.items():
        with pytest.raises(qlx.QlError, match="status -6.*not a qlx head checkpoint"):
            B.head.read_checkpoint(path)
        assert_same_state(head_state(B), before)
    with pytest.raises(qlx.QlError, match="cannot open"):
        B.head.read_checkpoint(str(tmp_path / "missing.ckpt"))
    assert_same_state(head_state(B), before)
    for T in (A, B, other):
        T.sync()
        T.close()
