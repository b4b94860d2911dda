"""Shared by tests/test_gpu_head_eval.py and tests/test_gpu_torch_head_eval.py: device arrays, a small world
of play to read states from, one deterministic train_dist update and a byte-level read-out of a net with its head."""
import numpy as np
import torch

import qlx_torch as QT   # before any other use of qlx in this process (it checks that itself)
import qlx

SEED = 0x51A5EED
DEV = "cuda:0"
LAY = "nchw_time"
N_ENVS, CAP, STEPS = 5, 256, 30
P_ACT_DEV = 9


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def host(t):
    return t.cpu().numpy()


def dev(a):
    return torch.as_tensor(np.array(a, order="C")).to(DEV)


def net(seed=5, reserve=128):
    return QT.TorchQNet("f32", seed=seed, device=DEV, reserve=reserve)


def make_dist(kind, N):
    return QT.Quantile(N) if kind == "quantile" else QT.Categorical(N, -10.0, 10.0)


def make_world():
    """5 envs, 30 vector steps into a replay of 256: 150 transitions of play, two envs reset on the way"""
    env = QT.TorchEnv(N_ENVS, SEED, DEV)
    rb = QT.TorchReplay(CAP, env)
    rng = np.random.default_rng(17)
    for t in range(STEPS):
        a = dev(rng.integers(0, 3, N_ENVS).astype(np.uint8))
        r, d = env.step(a)
        rb.add(env, a, r, d)
        if t in (9, 20):
            env.reset(dev(np.array([t == 9, 0, t == 20, 0, 0], np.uint8)))
    rb.sync()
    assert len(rb) == N_ENVS * STEPS
    return env, rb


def indices(world, n, seed=0):
    return dev(np.random.default_rng(1000 + seed).permutation(len(world[1]))[:n].astype(np.int64))


def update(T, world, dist, k, B=24):
    """update k of a fixed sequence (the same batch for every net that asks for update k): the loss on the host"""
    rng = np.random.default_rng(500 + k)
    if isinstance(dist, QT.Quantile):
        z_next = (1.5 * rng.normal(size=(B, dist.width))).astype(np.float32)
    else:
        z_next = (3.0 * rng.normal(size=(B, dist.width))).astype(np.float32)
    loss, _ = T.train_dist(dist, dev(rng.integers(0, 3, B).astype(np.uint8)), dev(rng.normal(size=B).astype(np.float32)),
                           dev(np.full(B, 0.99, np.float32)), dev((rng.random(B) < 0.2).astype(np.uint8)), dev(z_next),
                           replay=world[1], indices=indices(world, B, k), layout=LAY)
    return host(loss)


def head_state(T):
    """Wh, bh, their m and v, and the head's iterations"""
    return [T.head.get(var, which) for which in range(3) for var in range(2)] + [np.int64(T.head.iterations())]


def full_state(T):
    """the ten model variables with their Adam slots, the model's iterations, then head_state"""
    return ([T.model.get(v, which) for which in range(3) for v in range(qlx.NUM_VARS)] + [np.int64(T.model.iterations())]
            + head_state(T))


def assert_same_state(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert same(x, y), i


def summary_lists(s):
    return {k: np.asarray(v).tolist() for k, v in s.items()}
