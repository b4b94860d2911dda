"""n-step returns (qlx_params.n_step, qlx_replay_nstep; DESIGN.md §6 "n-step returns") on the GPU.

The reference here is a numpy float32 restatement of the window walk: numpy's float32 * float32 and float32 + float32
round once each, as __fmul_rn / __fadd_rn do, so every comparison is by bit pattern.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GAMMA = np.float32(0.99)
N_VALUES = (1, 2, 3, 5, 8, 32)


def _qlx():
    import qlx
    return qlx


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def ref_window(reward, done, epstep, N, p, n, gamma):
    """The window of the transition at push position p over the push-order logs (total = their length):
    (R, g, m, last push position, terminal, stop reason)"""
    total = len(reward)
    g, R, m, q = np.float32(1.0), np.float32(0.0), 0, p
    while True:
        r = np.float32(reward[q])
        R = r if m == 0 else np.float32(R + np.float32(g * r))
        g = np.float32(g * gamma)
        m += 1
        if m == n:
            why = "full"
            break
        if done[q]:
            why = "done"
            break
        if q + N >= total:
            why = "edge"
            break
        if epstep[q + N] != epstep[q] + 1:
            why = "cut"
            break
        q += N
    return R, g, m, q, bool(done[q]), why


def ref_windows(reward, done, epstep, N, length, n, gamma):
    """ref_window for every logical index 0 .. length - 1"""
    base = len(reward) - length
    rows = [ref_window(reward, done, epstep, N, base + i, n, gamma) for i in range(length)]
    return dict(returns=np.array([r[0] for r in rows], np.float32), discounts=np.array([r[1] for r in rows], np.float32),
                steps=np.array([r[2] for r in rows], np.uint32), last_indices=np.array([r[3] - base for r in rows], np.uint64),
                terminals=np.array([r[4] for r in rows], bool), why=[r[5] for r in rows])


def synth_draws(seed, T, N):
    """the random part of the walk test's data: actions, stored rewards, extra dones (p = 0.15), cuts without done (p = 0.1)"""
    rng = np.random.default_rng(seed)
    return dict(actions=rng.integers(0, 3, (T, N)).astype(np.uint8), rewards=rng.standard_normal((T, N)).astype(np.float32),
                dones=rng.random((T, N)) < 0.15, cuts=rng.random((T, N)) < 0.1)


WALK_SEED = 11   # with the env's own dones all False (20 Breakout steps end no game) every stop reason occurs at n = 3


@pytest.mark.parametrize("cap", [60, 37])
def test_window_walk_matches_numpy(cap):
    """qlx_replay_nstep over every live index of a wrapped ring (capacity a multiple of n_envs, and not), with episodes
    ended by done and cut without one, against the numpy walk; n = 1 is get_many's (reward, gamma, index, done)."""
    qlx = _qlx()
    N, T = 5, 20
    env = qlx.BreakoutEnvironment(n_envs=N)
    rb = qlx.ReplayBuffer(cap, N)
    draws = synth_draws(WALK_SEED, T, N)
    ep = np.zeros(N, np.uint32)
    reward, done, epstep = [], [], []
    for t in range(T):
        _, _, d_env = env.step(draws["actions"][t])
        d = d_env | draws["dones"][t]
        rb.add(env, draws["actions"][t], draws["rewards"][t], d)
        ep += 1
        reward.extend(draws["rewards"][t]); done.extend(d); epstep.extend(ep)
        mask = d | draws["cuts"][t]
        if mask.any():
            env.reset(mask.astype(np.uint8))
            ep[mask] = 0
    length = len(rb)
    assert length == cap and T * N > cap
    reward, done, epstep = np.array(reward, np.float32), np.array(done, bool), np.array(epstep, np.int64)
    idx = np.arange(length, dtype=np.uint64)
    for n in N_VALUES:
        ref = ref_windows(reward, done, epstep, N, length, n, GAMMA)
        got = rb.nstep(idx, n, float(GAMMA))
        for k in ("returns", "discounts", "last_indices", "terminals", "steps"):
            assert same(got[k], ref[k]), f"{k} differ at n = {n}"
        if n == 3:
            assert set(ref["why"]) == {"full", "done", "cut", "edge"}, sorted(set(ref["why"]))
        if n == 1:
            meta = rb.get_many(idx)
            assert same(got["returns"], meta["reward"]) and same(got["terminals"], meta["done"])
            assert same(got["discounts"], np.full(length, GAMMA, np.float32))
            assert same(got["last_indices"], idx) and same(got["steps"], np.ones(length, np.uint32))
    for bad in (0, 33):
        with pytest.raises(qlx.QlError):
            rb.nstep(idx[:4], bad, float(GAMMA))
    with pytest.raises(qlx.QlError):
        rb.nstep(np.array([0, length], np.uint64), 3, float(GAMMA))


LEARNER_CASES = {"memo": {}, "no_memo": {"cache": "0"}, "ddqn": {"flags": 1}, "target_sync": {"sync": 4}, "per_ddqn": {"flags": 3}}


@pytest.mark.parametrize("case", sorted(LEARNER_CASES))
def test_learner_targets_bit_exact(monkeypatch, case):
    """The learner's targets at n_step = 3 are where(terminal, R, R + v * g) bit for bit, with R, g, terminal and the
    window's last transition from qlx_replay_nstep and v the target net's bootstrap value at s' of that transition
    (double DQN: its Q at the first argmax of the online net as it stood before the step), through the memo, the
    per-batch pass, double DQN, target sync and PER.  The replay wraps and max_steps_per_episode cuts episodes.
    The target net the step used is the one before the step (a sync happens at the end of a vector step), so v comes
    from a copy of the stabilized model taken before the step."""
    qlx = _qlx()
    cfg = LEARNER_CASES[case]
    N, B, n = 16, 32, 3
    if "cache" in cfg:
        monkeypatch.setenv("QLX_TARGET_CACHE", cfg["cache"])
    else:
        monkeypatch.delenv("QLX_TARGET_CACHE", raising=False)
    ddqn = bool(cfg.get("flags", 0) & qlx.DOUBLE_DQN)
    p = qlx.Parameter(n_envs=N, batch_size=B, history_buffer_len=1000, update_after_actions=8, max_steps_per_episode=45,
                      epsilon_pure_random_steps=400, stats_after_steps=0, n_step=n, flags=cfg.get("flags", 0),
                      target_sync_steps=cfg.get("sync", 0) * N)
    L = qlx.SelfDrivingQLearner(p)
    online0, target0 = qlx.DeepQLearningModel(), qlx.DeepQLearningModel()
    gamma = np.float32(p.gamma)
    checked = 0
    for step in range(70):
        online0.copy_from(L.model)
        target0.copy_from(L.stabilized_model)
        L.vector_step()
        g = L.last()
        if not len(g["losses"]):
            continue
        idx = g["indices"].ravel()
        w = L.replay_buffer.nstep(idx, n, float(gamma))
        sn = L.replay_buffer.get_many(w["last_indices"])["state_next"]
        if ddqn:
            a_star = online0.q_values(sn)[0].argmax(axis=1)   # first maximal index
            v = target0.q_values(sn)[0][np.arange(idx.size), a_star]
        else:
            v = target0.batch_predict_max_future_reward(sn)
        y = np.where(w["terminals"], w["returns"], w["returns"] + v * w["discounts"]).astype(np.float32)
        assert same(g["targets"].ravel(), y), f"targets differ @ vector step {step}"
        checked += idx.size
    assert checked > 60 * 2 * B and len(L.replay_buffer) == 1000


@pytest.mark.parametrize("prec", [0, 1])
def test_memo_matches_per_batch_pass_at_n3(monkeypatch, prec):
    """The memo of bootstrap values gives the same targets, losses and weights as the per-batch target pass at n_step = 3,
    in both precisions, across the ring wrap and a target-weight write mid-run (the memo is rebuilt)."""
    qlx = _qlx()
    N, B, ua, cap, steps, write_at = 64, 32, 8, 1000, 30, 18   # test_gpu_learner.py MEMO_SHAPES["tiny"]

    def run(cache):
        monkeypatch.setenv("QLX_TARGET_CACHE", "1" if cache else "0")
        p = qlx.Parameter(n_envs=N, batch_size=B, history_buffer_len=cap, update_after_actions=ua,
                          epsilon_pure_random_steps=400, epsilon_greedy_steps=2000.0, max_steps_per_episode=200,
                          stats_after_steps=0, qnet_precision=prec, n_step=3)
        L = qlx.SelfDrivingQLearner(p)
        out = []
        for v in range(steps):
            if v == write_at:
                w = L.stabilized_model.get(9)
                L.stabilized_model.set(9, (w + np.float32(0.01)).astype(np.float32))
            L.vector_step()
            g = L.last()
            out.append((g["targets"].copy(), g["losses"].copy()))
        return out, [L.model.get(v) for v in range(10)]

    memo, w_memo = run(True)
    plain, w_plain = run(False)
    assert sum(len(l) for _, l in memo) > 0
    for v, ((ym, lm), (yp, lp)) in enumerate(zip(memo, plain)):
        assert same(ym, yp), f"targets differ @ vector step {v}"
        assert same(lm, lp), f"losses differ @ vector step {v}"
    for a, b in zip(w_memo, w_plain):
        assert same(a, b)


def test_nstep_1_and_0_are_the_one_step_learner():
    """n_step = 1, n_step = 0 and a Parameter without the field set run the same learner: targets, losses, weights."""
    qlx = _qlx()
    kw = dict(n_envs=16, batch_size=32, history_buffer_len=500, update_after_actions=4, stats_after_steps=0)

    def run(**extra):
        L = qlx.SelfDrivingQLearner(qlx.Parameter(**kw, **extra))
        out = []
        for _ in range(10):
            L.vector_step()
            g = L.last()
            out.append((g["targets"].copy(), g["losses"].copy()))
        return out, [L.model.get(v) for v in range(10)]

    base, w_base = run()
    assert sum(len(l) for _, l in base) > 0
    for extra in (dict(n_step=1), dict(n_step=0)):
        got, w_got = run(**extra)
        for (yb, lb), (yg, lg) in zip(base, got):
            assert same(yb, yg) and same(lb, lg), extra
        for a, b in zip(w_base, w_got):
            assert same(a, b), extra


def test_refusals():
    qlx = _qlx()
    with pytest.raises(qlx.QlError, match="n_step"):
        qlx.SelfDrivingQLearner(qlx.Parameter(n_envs=16, batch_size=32, history_buffer_len=500, n_step=33))
    with pytest.raises(qlx.QlError, match="n_step"):
        qlx.BallGameLearner(qlx.Parameter(n_envs=16, batch_size=32, history_buffer_len=500, n_step=2))
