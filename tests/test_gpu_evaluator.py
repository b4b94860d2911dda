"""Policy evaluation on the GPU (qlx_evaluator, DESIGN.md "Policy evaluation") against a Python restatement of its
contract over the unchanged oracle: oracle.Env for the game, oracle.QNet(f32=True).forward for Q, the oracle's Philox
draws (purpose 8, c1 = env, c2 = vector step; the f64 from word 0, the random action from word 2).

Per vector step t and env e still playing: q = Q(obs_e); random = epsilon > 0 and epsilon > f64 draw; a = the u8 draw
if random else the first argmax; return and max_a q accumulate in fp32 in step order; an episode ends at done or at
max_steps steps, is recorded at [e][k], and the env resets; an env retires after K records.  The run ends at the first
poll (every P steps) that finds no env playing; the forward of a step runs over the envs counted at the last poll.

fp32 is bit-exact against the restatement, for every poll_steps and with compaction off (the fp32 kernels never depend
on the batch).  bf16 results with random weights may depend on the batch a sample is evaluated in, hence on poll_steps
and on the compaction switch: for bf16 only run-to-run determinism is required (and exactness where Q is exact in
bf16: the zero-weight model)."""
import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

P_EVAL = 8
ENV_SEED = 0x51A5EED


def _qlx():
    import qlx
    return qlx


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def restatement(q_of, n, K, max_steps, epsilon=0.0, env_seed=ENV_SEED, policy_seed=1, env_ids=None):
    """the contract, sequentially: records [n][K], the action counts, the number of random actions.
    q_of(list of [84][84][4]) -> [m][3] fp32; env_ids: restate these envs of a larger batch only (envs are independent)"""
    L = O.lib()
    ids = list(range(n)) if env_ids is None else list(env_ids)
    n = len(ids)
    envs = [O.Env(env_seed, i) for i in ids]
    ret, qsum = np.zeros(n, np.float32), np.zeros(n, np.float32)
    length, k = np.zeros(n, np.int64), np.zeros(n, np.int64)
    rec = dict(returns=np.zeros((n, K), np.float32), lengths=np.zeros((n, K), np.uint32),
               terminals=np.zeros((n, K), bool), max_q_sums=np.zeros((n, K), np.float32))
    counts = np.zeros(3, np.uint64)
    t = randoms = 0
    while (k < K).any():
        act = [e for e in range(n) if k[e] < K]
        q = np.asarray(q_of([envs[e].tensor() for e in act]), np.float32)
        for i, e in enumerate(act):
            random = epsilon > 0 and epsilon > L.orc_gen_f64_01(policy_seed, ids[e], t, P_EVAL)
            a = L.orc_gen_u8(policy_seed, ids[e], t, P_EVAL, 2, 3) if random else int(np.argmax(q[i]))
            randoms += int(random)
            r, done = envs[e].step(a)
            ret[e] += np.float32(r)
            qsum[e] += q[i].max()
            length[e] += 1
            counts[a] += 1
            if done or length[e] >= max_steps:
                rec["returns"][e, k[e]], rec["lengths"][e, k[e]] = ret[e], length[e]
                rec["terminals"][e, k[e]], rec["max_q_sums"][e, k[e]] = done, qsum[e]
                k[e] += 1
                ret[e] = qsum[e] = 0
                length[e] = 0
                envs[e].reset()
        t += 1
    return rec, counts, randoms


def expected_steps(lengths, P, compact=True):
    """(vector_steps, forward_samples): the run ends at the first poll with no env playing; the rows of a step are
    the envs still playing at the last poll (all n before the first, and always without compaction)"""
    T = lengths.astype(np.int64).sum(axis=1)
    polls = -(-int(T.max()) // P)
    fs = sum(P * (int((T > j * P).sum()) if compact else len(T)) for j in range(polls))
    return polls * P, fs


def check_summary(s, rec, counts, P, compact=True):
    flat = {k: v.reshape(-1) for k, v in rec.items()}
    steps = int(flat["lengths"].astype(np.int64).sum())
    seq = lambda x: float(sum(float(v) for v in x))   # double sums in [e][k] order
    assert s["episodes"] == flat["returns"].size
    assert s["env_steps"] == steps
    assert s["terminal_episodes"] == int(flat["terminals"].sum())
    assert s["mean_return"] == seq(flat["returns"]) / flat["returns"].size
    assert s["mean_length"] == steps / flat["returns"].size
    assert s["mean_max_q"] == seq(flat["max_q_sums"]) / steps
    assert s["min_return"] == flat["returns"].min() and s["max_return"] == flat["returns"].max()
    assert same(s["action_counts"], counts) and int(counts.sum()) == steps
    vs, fs = expected_steps(rec["lengths"], P, compact)
    assert (s["vector_steps"], s["forward_samples"]) == (vs, fs)


def assert_records(got, ref):
    for key in ("returns", "lengths", "terminals", "max_q_sums"):
        assert same(got[key], ref[key]), key


@pytest.fixture(scope="module")
def net7():
    """the fp32 product model of seed 7 and an oracle net with its weights"""
    qlx = _qlx()
    m = qlx.DeepQLearningModel(seed=7)
    ref = O.QNet(f32=True)
    ref.load_state_from(m)
    yield m, ref
    m.close()


GREEDY = dict(n_envs=6, episodes_per_env=2, max_steps_per_episode=162, epsilon=0.0, env_seed=ENV_SEED)
EPSILON = dict(n_envs=6, episodes_per_env=2, max_steps_per_episode=150, epsilon=0.25, env_seed=ENV_SEED, policy_seed=0xE7A1)
TAIL = dict(n_envs=16, episodes_per_env=1, max_steps_per_episode=1500, epsilon=0.0, env_seed=ENV_SEED)
TAIL_LENGTHS = [166, 163, 160, 537, 163, 160, 163, 164, 165, 160, 161, 162, 165, 164, 161, 1172]


def _ref(cfg, q_of):
    return restatement(q_of, cfg["n_envs"], cfg["episodes_per_env"], cfg["max_steps_per_episode"], cfg["epsilon"],
                       cfg["env_seed"], cfg.get("policy_seed", 1))


@pytest.fixture(scope="module")
def greedy_ref(net7):
    return _ref(GREEDY, net7[1].forward)


@pytest.fixture(scope="module")
def tail_ref():
    return _ref(TAIL, lambda xs: np.tile(np.float32([1, 0, 0]), (len(xs), 1)))


def zero_model(precision):
    """all weights and biases zero but b4 = [1, 0, 0]: Q = b4 exactly in fp32 and bf16, the policy is action 0"""
    qlx = _qlx()
    m = qlx.DeepQLearningModel(seed=1, precision=precision)
    for v, shape in enumerate(qlx.VAR_SHAPES):
        m.set(v, np.zeros(shape, np.float32))
    m.set(9, np.float32([1, 0, 0]))
    return m


def run(cfg, model, poll_steps=8):
    qlx = _qlx()
    ev = qlx.Evaluator(poll_steps=poll_steps, **cfg)
    try:
        s = ev.run(model)
        return s, ev.episodes()
    finally:
        ev.close()


def test_f32_greedy_parity(net7, greedy_ref):
    rec, counts, _ = greedy_ref
    # the case covers both end reasons and unequal retire times
    assert rec["terminals"].any() and not rec["terminals"].all()
    assert len(set(rec["lengths"].sum(axis=1).tolist())) > 1
    s, got = run(GREEDY, net7[0])
    assert_records(got, rec)
    check_summary(s, rec, counts, 8)


def test_f32_epsilon_parity(net7):
    rec, counts, randoms = _ref(EPSILON, net7[1].forward)
    assert 0.15 * counts.sum() < randoms < 0.35 * counts.sum()   # the draw path is exercised
    s, got = run(EPSILON, net7[0])
    assert_records(got, rec)
    check_summary(s, rec, counts, 8)


@pytest.mark.parametrize("precision", [0, 1], ids=["f32", "bf16"])
def test_long_tail_compaction(tail_ref, precision):
    rec, counts, _ = tail_ref
    assert rec["lengths"][:, 0].tolist() == TAIL_LENGTHS
    assert rec["returns"][:, 0].tolist() == [2.0 if e in (3, 15) else 1.0 for e in range(16)]
    m = zero_model(precision)
    try:
        s, got = run(TAIL, m)
    finally:
        m.close()
    assert_records(got, rec)
    check_summary(s, rec, counts, 8)
    assert s["vector_steps"] == 1176
    assert s["forward_samples"] < 16 * s["vector_steps"] / 4
    assert s["action_counts"].tolist() == [sum(TAIL_LENGTHS), 0, 0]


@pytest.mark.parametrize("case", ["greedy", "tail"])
def test_switch_equivalence_f32(net7, greedy_ref, tail_ref, case, monkeypatch):
    cfg, (rec, counts, _) = (GREEDY, greedy_ref) if case == "greedy" else (TAIL, tail_ref)
    m = net7[0] if case == "greedy" else zero_model(0)
    try:
        for P in (1, 32):
            s, got = run(cfg, m, poll_steps=P)
            assert_records(got, rec)
            check_summary(s, rec, counts, P)
        monkeypatch.setenv("QLX_EVAL_COMPACT", "0")   # read once at qlx_evaluator_create
        s, got = run(cfg, m)
        assert_records(got, rec)
        check_summary(s, rec, counts, 8, compact=False)
        assert s["forward_samples"] == cfg["n_envs"] * s["vector_steps"]
    finally:
        if case == "tail":
            m.close()


def test_compaction_over_several_rounds_f32(net7, monkeypatch):
    """More than 1,024 envs: the book kernel's running offset over its rounds of 1,024, with envs retiring at different
    steps on both sides of the round boundary.  The records do not depend on poll_steps or on compaction (fp32), the
    summary follows from them, and a few envs around the boundary match the oracle restatement."""
    cfg = dict(n_envs=1100, episodes_per_env=1, max_steps_per_episode=161, epsilon=0.05, env_seed=ENV_SEED, policy_seed=9)
    s1, r1 = run(cfg, net7[0], poll_steps=1)
    s8, r8 = run(cfg, net7[0], poll_steps=8)
    monkeypatch.setenv("QLX_EVAL_COMPACT", "0")
    s0, r0 = run(cfg, net7[0], poll_steps=8)
    assert_records(r8, r1)
    assert_records(r0, r1)
    T = r1["lengths"][:, 0]
    assert len(set(T[:1024].tolist())) > 2 and len(set(T[1024:].tolist())) > 2 and T.max() == 161
    assert r1["terminals"].any() and not r1["terminals"].all()
    for s, P, compact in ((s1, 1, True), (s8, 8, True), (s0, 8, False)):
        check_summary(s, r1, s1["action_counts"], P, compact)
    ids = [0, 1023, 1024, 1099]
    rec, _, _ = restatement(net7[1].forward, None, 1, 161, 0.05, ENV_SEED, 9, env_ids=ids)
    assert_records({k: v[ids] for k, v in r1.items()}, rec)


def test_max_envs_f32(net7, monkeypatch):
    """QLX_EVAL_MAX_ENVS envs: eight rounds of the book kernel, and a forward that starts on the fp32 kernels for batches
    above 2,048 and shrinks onto the small-batch ones.  Same records with and without compaction; envs at the ends and on
    both sides of 2,048 match the oracle restatement."""
    cfg = dict(n_envs=8192, episodes_per_env=1, max_steps_per_episode=161, epsilon=0.0, env_seed=ENV_SEED)
    s8, r8 = run(cfg, net7[0], poll_steps=8)
    monkeypatch.setenv("QLX_EVAL_COMPACT", "0")
    s0, r0 = run(cfg, net7[0], poll_steps=8)
    assert_records(r0, r8)
    assert len(set(r8["lengths"][:, 0].tolist())) > 2
    check_summary(s8, r8, s8["action_counts"], 8)
    check_summary(s0, r8, s8["action_counts"], 8, compact=False)
    assert s8["forward_samples"] < s0["forward_samples"]
    ids = [0, 2047, 2048, 8191]
    rec, _, _ = restatement(net7[1].forward, None, 1, 161, env_ids=ids)
    assert_records({k: v[ids] for k, v in r8.items()}, rec)


def test_single_env_f32(net7):
    """one env, one forward row: three short episodes at epsilon 0.5"""
    cfg = dict(n_envs=1, episodes_per_env=3, max_steps_per_episode=7, epsilon=0.5, env_seed=3, policy_seed=4)
    rec, counts, randoms = _ref(cfg, net7[1].forward)
    assert 0 < randoms < 21
    s, got = run(cfg, net7[0], poll_steps=2)
    assert_records(got, rec)
    check_summary(s, rec, counts, 2)
    assert s["vector_steps"] == 22 and s["forward_samples"] == 22   # 21 steps, the next poll at 22


@pytest.mark.parametrize("precision", [0, 1], ids=["f32", "bf16"])
def test_determinism_and_model_untouched(precision):
    """Two runs of one evaluator and a run of a fresh one give identical records and summaries; the model's weights,
    Adam slots and iteration count are what they were.  (The only bf16 requirement with random weights: bf16 results
    may depend on the batch a sample is evaluated in, hence on poll_steps.)"""
    qlx = _qlx()
    cfg = dict(n_envs=6, episodes_per_env=2, max_steps_per_episode=40, epsilon=0.1, env_seed=ENV_SEED, policy_seed=5)
    m = qlx.DeepQLearningModel(seed=7, precision=precision)
    rng = np.random.default_rng(3)
    for v, shape in enumerate(qlx.VAR_SHAPES):   # distinguishable Adam slots
        m.set(v, rng.standard_normal(shape).astype(np.float32) * 1e-3, which=1)
        m.set(v, rng.random(shape).astype(np.float32) * 1e-6, which=2)
    before = [[m.get(v, w) for w in range(3)] for v in range(10)]
    it = m.iterations()
    ev = qlx.Evaluator(poll_steps=4, **cfg)
    try:
        s1, r1 = ev.run(m), ev.episodes()
        s2, r2 = ev.run(m), ev.episodes()
    finally:
        ev.close()
    s3, r3 = run(cfg, m, poll_steps=4)
    for s, r in ((s2, r2), (s3, r3)):
        assert_records(r, r1)
        assert {k: np.asarray(v).tolist() for k, v in s.items()} == {k: np.asarray(v).tolist() for k, v in s1.items()}
    assert s1["episodes"] == 12 and s1["env_steps"] == int(r1["lengths"].sum()) and r1["lengths"].max() <= 40
    assert m.iterations() == it
    for v in range(10):
        for w in range(3):
            assert same(m.get(v, w), before[v][w]), (v, w)
    m.close()


@pytest.mark.parametrize("precision", [0, 1], ids=["f32", "bf16"])
def test_learner_is_undisturbed(precision):
    """Two identical learners; one evaluates its online model between vector steps with more envs than its own (the
    online model's workspace regrows).  Everything the two then compute is bit-identical."""
    qlx = _qlx()
    kw = dict(n_envs=16, batch_size=32, history_buffer_len=2048, update_after_actions=4, epsilon_pure_random_steps=32,
              epsilon_max=0.5, epsilon_min=0.05, epsilon_greedy_steps=500.0, max_steps_per_episode=10_000,
              stats_after_steps=0, qnet_precision=precision)
    a = qlx.SelfDrivingQLearner(qlx.Parameter(**kw))
    b = qlx.SelfDrivingQLearner(qlx.Parameter(**kw))
    cfg = dict(n_envs=24, episodes_per_env=1, max_steps_per_episode=12, epsilon=0.05, env_seed=11, policy_seed=12,
               poll_steps=4)
    try:
        a.run(6)
        b.run(6)
        s = a.evaluate(**cfg)
        assert s["episodes"] == 24 and s["vector_steps"] == 12 and s["env_steps"] == 24 * 12
        if precision == 0:   # evaluate = an Evaluator run of the online model with the same config
            ev = qlx.Evaluator(**cfg)
            try:
                s2 = ev.run(a.model)
            finally:
                ev.close()
            assert {k: np.asarray(v).tolist() for k, v in s.items()} == {k: np.asarray(v).tolist() for k, v in s2.items()}
        updates = 0
        for v in range(4):
            a.vector_step()
            b.vector_step()
            la, lb = a.last(), b.last()
            for k in ("actions", "rewards", "dones", "losses", "indices", "targets"):
                assert same(la[k], lb[k]), (k, v)
            updates += len(la["losses"])
            assert same(a.environment.hashes(), b.environment.hashes())
            assert same(a.environment.mechanics(), b.environment.mechanics())
            assert a.stats() == b.stats()
        assert updates == 16
        for ma, mb in ((a.model, b.model), (a.stabilized_model, b.stabilized_model)):
            assert ma.iterations() == mb.iterations()
            for var in range(10):
                for which in range(3):
                    assert same(ma.get(var, which), mb.get(var, which)), (var, which)
    finally:
        a.close()
        b.close()
