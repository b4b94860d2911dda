"""TorchQNet.act / select / evaluate / save_head / load_head (q-learning_amd/qlx_torch.py) against the C calls
they wrap, as bits; their misuse checks; and scripts/torch_qrdqn_example.py with --act-fused --eval in a process of its own."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from head_eval_helpers import (DEV, LAY, QT, assert_same_state, dev, head_state, host, indices, make_dist, make_world, net,
                               qlx, same, summary_lists, update)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 51


@pytest.fixture(scope="module")
def world():
    w = make_world()
    yield w
    w[1].close()
    w[0].close()


def c_select(T, dist, z, epsilon, seed, step):
    n = z.shape[0]
    a = torch.empty(n, dtype=torch.uint8, device=DEV)
    mq = torch.empty(n, dtype=torch.float32, device=DEV)
    q = torch.empty((n, 3), dtype=torch.float32, device=DEV)
    T._run(None, None, (z, a, mq, q),
           lambda: qlx.lib().qlx_head_select_dev(T.head.h, C.byref(dist.c), z.data_ptr(), n, epsilon, seed, step, a.data_ptr(),
                                                 mq.data_ptr(), q.data_ptr()))
    return dict(actions=host(a), max_q=host(mq), q=host(q))


@pytest.mark.parametrize("kind", ["quantile", "categorical"])
def test_select_and_act_are_the_c_calls(world, kind):
    env, rb = world
    T = net()
    T.attach_head(3 * N, seed=8)
    dist = make_dist(kind, N)
    z = dev((2.0 * np.random.default_rng(4).normal(size=(37, 3 * N))).astype(np.float32))
    ref = c_select(T, dist, z, 0.25, 3, 14)
    a, mq, q = T.select(z, dist, 0.25, 3, 14, want=("actions", "max_q", "q"))
    assert same(host(a), ref["actions"]) and same(host(mq), ref["max_q"]) and same(host(q), ref["q"])
    assert same(host(T.select(z, dist, 0.25, 3, 14)), ref["actions"])                       # the default: actions alone
    assert same(host(T.select(z, dist, 0.25, 3, 14, want="max_q")), ref["max_q"])
    out = dict(q=torch.zeros((37, 3), dtype=torch.float32, device=DEV))
    got = T.select(z, dist, 0.25, 3, 14, want=("q",), out=out)
    assert got[0] is out["q"] and same(host(out["q"]), ref["q"])
    greedy = T.head_values(z, dist, want="actions")
    assert same(host(T.select(z, dist, 0.0, 3, 14)), host(greedy))
    assert len(set(ref["actions"].tolist())) > 1 and (ref["actions"] != host(greedy)).any()
    # act over the env's ring and over replay indices: the forward, then select
    for src in (dict(env=env), dict(replay=rb, indices=indices(world, 100, 2))):
        t0 = T.forward_ticket()
        a, mq, q = T.act(dist, 0.25, 3, 15, layout=LAY, want=("actions", "max_q", "q"), **src)
        assert T.forward_ticket() == t0 + 1
        with torch.no_grad():
            _, zz = T.forward(head=True, layout=LAY, **src)
        ref = c_select(T, dist, zz, 0.25, 3, 15)
        assert same(host(a), ref["actions"]) and same(host(mq), ref["max_q"]) and same(host(q), ref["q"])
        n = zz.shape[0]
        assert same(host(T._act_work[3 * N][:n]), host(zz))   # the work tensor holds Z, and is kept
        work = T._act_work[3 * N]
        assert same(host(T.act(dist, 0.25, 3, 15, layout=LAY, **src)), ref["actions"]) and T._act_work[3 * N] is work
    T.sync()
    T.close()


def test_evaluate_and_head_checkpoints(world, tmp_path):
    dist = make_dist("quantile", N)
    T = net(seed=7)
    T.attach_head(3 * N, seed=21)
    update(T, world, dist, 0)
    cfg = dict(n_envs=6, episodes_per_env=1, max_steps_per_episode=40, epsilon=0.1, policy_seed=5, poll_steps=4)
    ev = qlx.Evaluator(**cfg)
    try:
        s_head, r_head = T.evaluate(ev, dist), ev.episodes()
        ref = ev.run_head(T.head, dist.c)
        assert summary_lists(s_head) == summary_lists(ref)
        assert all(same(r_head[k], v) for k, v in ev.episodes().items())
        s_plain = T.evaluate(ev)
        assert summary_lists(s_plain) == summary_lists(ev.run(T.model))
        assert s_head["episodes"] == s_plain["episodes"] == 6 and s_head["mean_max_q"] != s_plain["mean_max_q"]
        with pytest.raises(ValueError, match="Evaluator"):
            T.evaluate(T.model, dist)
        with pytest.raises(ValueError, match="width"):
            T.evaluate(ev, QT.Quantile(50))
    finally:
        ev.close()
    path = str(tmp_path / "head.ckpt")
    assert T.save_head(path) == path
    U = net(seed=9)
    U.attach_head(3 * N, seed=1)
    U.load_head(path)
    assert_same_state(head_state(U), head_state(T))
    assert U.head.iterations() == 1
    plain = net()
    for call in (lambda: plain.save_head(path), lambda: plain.load_head(path), lambda: plain.evaluate(qlx.Evaluator(2), dist)):
        with pytest.raises(RuntimeError, match="attach_head"):
            call()
    for X in (T, U, plain):
        X.sync()
        X.close()


def test_misuse_is_refused_before_anything_runs(world):
    env, _ = world
    T = net(reserve=16)
    dist = make_dist("quantile", N)
    z = torch.zeros((4, 3 * N), dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="attach_head"):
        T.select(z, dist, 0.1, 1, 0)
    with pytest.raises(RuntimeError, match="attach_head"):
        T.act(dist, 0.1, 1, 0, env=env)
    T.attach_head(3 * N)
    ticket = T.forward_ticket()
    bad = [
        lambda: T.select(z, "quantile", 0.1, 1, 0),                                  # not a Quantile / Categorical
        lambda: T.select(z, QT.Quantile(50), 0.1, 1, 0),                             # another width
        lambda: T.select(z.double(), dist, 0.1, 1, 0),                               # dtype
        lambda: T.select(z.cpu(), dist, 0.1, 1, 0),                                  # device
        lambda: T.select(z[:, :-1], dist, 0.1, 1, 0),                                # shape
        lambda: T.select(z[0], dist, 0.1, 1, 0),                                     # not 2-d
        lambda: T.select(torch.zeros((17, 3 * N), dtype=torch.float32, device=DEV), dist, 0.1, 1, 0),   # above the reserve
        lambda: T.select(z, dist, float("nan"), 1, 0),
        lambda: T.select(z, dist, 1.5, 1, 0),
        lambda: T.select(z, dist, -0.1, 1, 0),
        lambda: T.select(z, dist, 0.1, 1, 0, want=()),                               # a want that names nothing
        lambda: T.select(z, dist, 0.1, 1, 0, want="values"),
        lambda: T.select(z, dist, 0.1, 1, 0, want="actions", out=dict(q=z)),          # out names what want does not
        lambda: T.select(z, dist, 0.1, 1, 0, out=dict(actions=torch.zeros(4, dtype=torch.float32, device=DEV))),
        lambda: T.act(dist, 0.1, 1, 0),                                              # no source
        lambda: T.act(dist, 0.1, 1, 0, env=env, obs=torch.zeros((4, 4, 84, 84), dtype=torch.uint8, device=DEV)),
        lambda: T.act(dist, float("nan"), 1, 0, env=env),
        lambda: T.act(dist, 0.1, 1, 0, env=env, want=()),
        lambda: T.act(QT.Quantile(50), 0.1, 1, 0, env=env),
        lambda: T.act(dist, 0.1, 1, 0, obs=torch.zeros((17, 4, 84, 84), dtype=torch.uint8, device=DEV)),   # above the reserve
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
    assert T.forward_ticket() == ticket and not T._act_work
    T.sync()
    T.close()


@pytest.mark.parametrize("flags", [["--fused"], ["--c51", "--fused"]], ids=["qrdqn", "c51"])
def test_example_acts_fused_and_evaluates(flags):
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "torch_qrdqn_example.py"), "--envs", "32", "--updates", "20", "--batch", "16",
           "--replay", "2000", "--warmup-steps", "5", "--act-fused", "--eval", "8", "--eval-max-steps", "200"] + flags
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "done (" in p.stdout and "20 updates" in p.stdout
    line = [x for x in p.stdout.splitlines() if x.startswith("evaluation (greedy, 8 envs")]
    assert len(line) == 1 and "mean return" in line[0], p.stdout
