"""Per-update training metrics (qlx_update_metrics rows written by one kernel per update into a ring in device memory).

fp32 rows are checked field by field against a numpy restatement: before each vector step the online weights go into a
spare model, after it the step's batch (indices and targets from last(), states and actions from the replay) is pushed
through the spare model, whose fp32 Q values do not depend on the batch they are evaluated in - so they are the training
head's bits.  Integer fields, minima, maxima, the loss and the gradient norms must be equal bit for bit; each mean must
be within one fp32 ulp of the float64 numpy mean (a double sum of B <= 4096 floats errs by at most B * 2^-53 * mean|x|,
far below half an fp32 ulp, so only the final rounding can differ).  bf16 and BallGame rows, whose Q values cannot be
restated that way, are checked for their invariants, for what last() does report, and for run-to-run identity; and a
learner with metrics on must compute exactly what one with metrics off computes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
MEANS = ("q_taken_mean", "q_max_mean", "action_gap_mean", "y_mean", "td_abs_mean", "weight_mean")


def _qlx():
    import qlx
    return qlx


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def global_norm(norms):
    s = 0.0
    for v in norms:   # v ascending, in double
        s += float(v) * float(v)
    return F32(np.sqrt(s))


def restate(qlx, q, actions, y, w):
    """the float and count fields of a row from the batch's Q values [B][A], actions, targets and IS weights"""
    q, y, w = np.asarray(q, F32), np.asarray(y, F32), np.asarray(w, F32)
    B = q.shape[0]
    rows = np.arange(B)
    qa = q[rows, actions]
    td = np.abs(qa - y)
    first = q.argmax(axis=1)   # first maximal index
    top = q[rows, first]
    rest = q.copy()
    rest[rows, first] = -np.inf
    gap = top - rest.max(axis=1)
    exact = dict(q_taken_min=qa.min(), q_taken_max=qa.max(), y_min=y.min(), y_max=y.max(), td_abs_max=td.max())
    means = dict(q_taken_mean=qa, q_max_mean=top, action_gap_mean=gap, y_mean=y, td_abs_mean=td, weight_mean=w)
    counts = dict(n_linear=int((td > 1).sum()),
                  argmax_counts=np.bincount(first, minlength=8).astype(np.uint32),
                  td_hist=np.bincount([qlx.metrics_td_bin(t) for t in td], minlength=16).astype(np.uint32))
    return exact, {k: np.mean(v.astype(np.float64)) for k, v in means.items()}, counts


def check_norm_fields(qlx, row, n_vars):
    clipnorm = qlx.model_hparams()[4]
    norms = row["grad_norm"]
    assert not norms[n_vars:].any() and np.isfinite(norms).all()
    assert row["n_clipped"] == int((norms[:n_vars] > clipnorm).sum())
    assert same(row["grad_norm_global"], global_norm(norms[:n_vars]))


def check_row(qlx, row, q, actions, y, w, loss, norms=None):
    """the full check of an fp32 Breakout row against the restatement"""
    B = len(actions)
    assert (row["batch"], row["n_actions"], row["n_vars"], row["reserved"], row["n_nonfinite"]) == (B, 3, 10, 0, 0)
    assert same(row["loss"], F32(loss))
    exact, means, counts = restate(qlx, q, actions, y, w)
    for k, v in exact.items():
        assert same(row[k], F32(v)), (k, row[k], v)
    for k, m in means.items():
        assert abs(np.float64(row[k]) - m) <= abs(np.float64(np.spacing(F32(m)))), (k, row[k], m)
    assert row["n_linear"] == counts["n_linear"]
    assert same(row["argmax_counts"], counts["argmax_counts"]) and same(row["td_hist"], counts["td_hist"])
    if norms is not None:
        assert same(row["grad_norm"][:10], np.asarray(norms, F32))
    check_norm_fields(qlx, row, 10)


def check_invariants(qlx, row, B, n_actions, n_vars, loss, per=False):
    assert (row["batch"], row["n_actions"], row["n_vars"], row["reserved"], row["n_nonfinite"]) == (B, n_actions, n_vars, 0, 0)
    assert row["td_hist"].sum() == B and row["argmax_counts"].sum() == B and not row["argmax_counts"][n_actions:].any()
    assert row["q_taken_min"] <= row["q_taken_mean"] <= row["q_taken_max"]
    assert row["y_min"] <= row["y_mean"] <= row["y_max"]
    assert 0 <= row["td_abs_mean"] <= row["td_abs_max"] and row["n_linear"] <= B
    assert row["q_taken_mean"] <= row["q_max_mean"] and row["action_gap_mean"] >= 0
    assert same(row["loss"], F32(loss))
    if not per:
        assert row["weight_mean"] == 1.0
    check_norm_fields(qlx, row, n_vars)


def breakout_params(qlx, **kw):
    p = dict(n_envs=16, batch_size=32, history_buffer_len=1000, update_after_actions=16, max_steps_per_episode=45,
             epsilon_pure_random_steps=400, stats_after_steps=0)
    p.update(kw)
    return qlx.Parameter(**p)


def check_step(qlx, L, spare, rows, per, norms_too):
    """rows = the rows of the vector step L just ran (spare holds the online weights from before it): counters and
    losses of every row, the full check of the first"""
    g, st = L.last(), L.stats()
    U = len(g["losses"])
    assert len(rows) == U > 0
    assert same(rows["update"], np.arange(st["update_count"] - U, st["update_count"], dtype=np.uint64))
    assert (rows["step_count"] == st["step_count"]).all()
    assert same(rows["loss"], g["losses"])
    idx, y = g["indices"][0], g["targets"][0]
    meta = L.replay_buffer.get_many(idx)
    q = spare.q_values(meta["state"])[0]
    w = L.priorities()[0][0] if per else np.ones(len(idx), F32)
    norms = spare.train(meta["state"], meta["action"], y, want_grads=True)[2] if norms_too else None
    check_row(qlx, rows[0], q, meta["action"], y, w, g["losses"][0], norms)


def run_checked(qlx, p, steps, prefill=0):
    per = bool(p.flags & qlx.PER)
    L = qlx.SelfDrivingQLearner(p)
    spare = qlx.DeepQLearningModel()
    if prefill:
        L.prefill(prefill)
    L.metrics_enable(64)
    checked = 0
    for _ in range(steps):
        spare.copy_from(L.model)
        L.vector_step()
        rows, dropped = L.metrics()
        assert dropped == 0
        if not len(L.last()["losses"]):
            assert len(rows) == 0
            continue
        check_step(qlx, L, spare, rows, per, norms_too=not per)
        checked += len(rows)
    info = L.metrics_info()
    assert info == dict(capacity=64, recorded=checked, unread=0)
    return checked


@pytest.mark.parametrize("case", ["memo", "ddqn_per", "nstep3"])
def test_fp32_rows_match_the_restatement(case):
    qlx = _qlx()
    kw = {"memo": {}, "ddqn_per": dict(flags=3), "nstep3": dict(n_step=3)}[case]
    assert run_checked(qlx, breakout_params(qlx, **kw), steps=40) >= 36


@pytest.mark.parametrize("B", [1, 100, 257])
def test_ragged_batches(B):
    """B = 1 (every min, mean and max coincide), 100, and 257: one sample past the workgroup's width"""
    qlx = _qlx()
    assert run_checked(qlx, breakout_params(qlx, batch_size=B), steps=3, prefill=B // 16 + 1) == 3


def test_several_updates_per_step():
    qlx = _qlx()
    assert run_checked(qlx, breakout_params(qlx, update_after_actions=4), steps=12) >= 4 * 8


def test_ring():
    qlx = _qlx()
    L = qlx.SelfDrivingQLearner(breakout_params(qlx))
    with pytest.raises(qlx.QlError, match="status -4"):
        L.metrics_info()
    L.prefill(3)
    L.metrics_enable(4)
    assert L.metrics_info() == dict(capacity=4, recorded=0, unread=0)
    L.run(10)
    u1 = L.stats()["update_count"]
    assert u1 == 10
    assert L.metrics_info() == dict(capacity=4, recorded=10, unread=4)
    rows, dropped = L.metrics()
    assert dropped == 6 and same(rows["update"], np.arange(6, 10, dtype=np.uint64))
    assert L.metrics_info() == dict(capacity=4, recorded=10, unread=0)
    rows, dropped = L.metrics()
    assert len(rows) == 0 and dropped == 0
    L.run(4)
    rows, dropped = L.metrics(max_rows=3)
    assert dropped == 0 and same(rows["update"], np.arange(10, 13, dtype=np.uint64))
    assert L.metrics_info() == dict(capacity=4, recorded=14, unread=1)
    L.run(5)   # the one unread row and one more are overwritten
    rows, dropped = L.metrics()
    assert dropped == 2 and same(rows["update"], np.arange(15, 19, dtype=np.uint64))
    L.metrics_enable(0)
    with pytest.raises(qlx.QlError, match="status -4"):
        L.metrics()
    with pytest.raises(qlx.QlError, match="status -4"):
        L.metrics_info()
    with pytest.raises(qlx.QlError, match="status -1"):
        L.metrics_enable(1 << 21)
    L.metrics_enable(8)   # recorded restarts, update carries on
    L.run(2)
    assert L.metrics_info() == dict(capacity=8, recorded=2, unread=2)
    rows, dropped = L.metrics()
    assert dropped == 0 and same(rows["update"], np.arange(19, 21, dtype=np.uint64))
    assert same(rows["loss"][-1:], L.last()["losses"])


def run_pair_undisturbed(make, var_count, steps=20):
    """two equal learners, metrics on in one: losses, targets, every variable and both Adam slots bit-identical"""
    on, off = make(), make()
    on.metrics_enable(16)
    updates = 0
    for _ in range(steps):
        on.vector_step()
        off.vector_step()
        a, b = on.last(), off.last()
        for k in ("actions", "rewards", "dones", "losses", "indices", "targets"):
            assert same(a[k], b[k]), k
        updates += len(a["losses"])
    assert updates > 0 and on.metrics_info()["recorded"] == updates
    for which in range(3):
        for v in range(var_count):
            assert same(on.model.get(v, which), off.model.get(v, which)), (v, which)


@pytest.mark.parametrize("prec", [0, 1])
def test_undisturbed(prec):
    qlx = _qlx()
    run_pair_undisturbed(lambda: qlx.SelfDrivingQLearner(breakout_params(qlx, update_after_actions=4, qnet_precision=prec)), 10)


def test_bf16_rows():
    qlx = _qlx()

    def run():
        L = qlx.SelfDrivingQLearner(breakout_params(qlx, update_after_actions=8, qnet_precision=qlx.PREC_BF16))
        L.metrics_enable(64)
        out = []
        for _ in range(20):
            L.vector_step()
            rows, dropped = L.metrics()
            losses = L.last()["losses"]
            assert dropped == 0 and len(rows) == len(losses)
            for r, loss in zip(rows, losses):
                check_invariants(qlx, r, 32, 3, 10, loss)
            out.append(rows)
        return np.concatenate(out)

    a, b = run(), run()
    assert len(a) >= 30 and a.tobytes() == b.tobytes()


def test_nonfinite_alarm():
    """b4[0] = +inf on the online model: Q(s)[0] is +inf for every sample, so exactly the samples whose action is 0 have a
    non-finite q_a; the target net is separate and never synced here, so y stays finite."""
    qlx = _qlx()
    L = qlx.SelfDrivingQLearner(breakout_params(qlx))
    L.prefill(3)
    L.metrics_enable(4)
    L.vector_step()
    rows, _ = L.metrics()
    assert len(rows) == 1 and rows[0]["n_nonfinite"] == 0
    b4 = L.model.get(9)
    b4[0] = np.inf
    L.model.set(9, b4)
    L.vector_step()
    g = L.last()
    rows, _ = L.metrics()
    assert len(rows) == 1 and np.isfinite(g["targets"]).all()
    act = L.replay_buffer.get_many(g["indices"][0])["action"]
    expect = int((act == 0).sum())
    assert 0 < expect < 32
    r = rows[0]
    assert r["n_nonfinite"] == expect
    assert r["td_hist"].sum() == 32 and r["td_hist"][15] >= expect and r["n_linear"] >= expect
    assert r["argmax_counts"][0] == 32 and r["q_taken_max"] == np.inf and r["td_abs_max"] == np.inf


def bg_learner(qlx, **kw):
    p = dict(n_envs=16, batch_size=32, history_buffer_len=1000, update_after_actions=8, epsilon_pure_random_steps=200,
             gamma=0.95)
    p.update(kw)
    return qlx.BallGameLearner(qlx.Parameter(**p))


def test_ballgame_rows():
    qlx = _qlx()

    def run():
        L = bg_learner(qlx)
        L.metrics_enable(64)
        out = []
        for _ in range(30):
            L.vector_step()
            rows, dropped = L.metrics()
            g, st = L.last(), L.stats()
            U = len(g["losses"])
            assert dropped == 0 and len(rows) == U
            assert same(rows["update"], np.arange(st["update_count"] - U, st["update_count"], dtype=np.uint64))
            for u, r in enumerate(rows):
                check_invariants(qlx, r, 32, 5, 8, g["losses"][u])
                y = g["targets"][u]
                assert r["step_count"] == st["step_count"]
                assert same(r["y_min"], y.min()) and same(r["y_max"], y.max())
                m = np.mean(y.astype(np.float64))
                assert abs(np.float64(r["y_mean"]) - m) <= abs(np.float64(np.spacing(F32(m))))
            out.append(rows)
        return np.concatenate(out)

    a, b = run(), run()
    assert len(a) >= 50 and a.tobytes() == b.tobytes()


def test_ballgame_undisturbed():
    qlx = _qlx()
    run_pair_undisturbed(lambda: bg_learner(qlx), 8)
