"""The distributional losses through qlx_torch.TorchQNet: head_values, dist_loss - plain and as an autograd
Function whose backward hands dz * grad on to forward(head=True)'s - and train_dist, against the C calls; the misuse
checks; and the example's two paths (scripts/torch_qrdqn_example.py, --fused and the loss in torch), which must run and
report a finite loss."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import qlx_torch as QT   # before any other use of qlx in this process (it checks that itself)
import qlx

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x51A5EED
DEV = "cuda:0"
LAY = "nchw_time"
N_ENVS, CAP, STEPS = 4, 128, 30
N = 51


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def host(t):
    return t.detach().cpu().numpy()


def dev(a):
    return torch.as_tensor(np.array(a, order="C")).to(DEV)


def net(seed=5, reserve=128):
    return QT.TorchQNet("f32", seed=seed, device=DEV, reserve=reserve)


@pytest.fixture(scope="module")
def world():
    env = QT.TorchEnv(N_ENVS, SEED, DEV)
    rb = QT.TorchReplay(CAP, env)
    rng = np.random.default_rng(17)
    for t in range(STEPS):
        a = dev(rng.integers(0, 3, N_ENVS).astype(np.uint8))
        r, d = env.step(a)
        rb.add(env, a, r, d)
        if t in (9, 20):
            env.reset(dev(np.array([t == 9, 0, t == 20, 0], np.uint8)))
    rb.sync()
    yield env, rb
    rb.close()
    env.close()


def source(world, B, seed=0):
    _, rb = world
    idx = np.random.default_rng(1000 + seed).permutation(len(rb))[:B].astype(np.int64)
    return dict(replay=rb, indices=dev(idx), layout=LAY)


def batch_args(rng, B, kind):
    """(actions, returns, discounts, terminals, z_next) on the device"""
    lo, hi = (-1.0, 1.0) if kind == "quantile" else (-12.0, 12.0)
    return (dev(rng.integers(0, 3, B).astype(np.uint8)), dev(rng.uniform(lo, hi, B).astype(np.float32)),
            dev(np.full(B, 0.97, np.float32)), dev((rng.random(B) < 0.2).astype(np.uint8)),
            dev(rng.normal(size=(B, 3 * N)).astype(np.float32)))


def dist_of(kind):
    return QT.Quantile(N) if kind == "quantile" else QT.Categorical(N, -10.0, 10.0)


@pytest.mark.parametrize("kind", ["quantile", "categorical"])
def test_methods_are_the_c_calls(world, kind):
    B = 33
    L = qlx.lib()
    T = net()
    head = T.attach_head(3 * N, seed=2)
    dist = dist_of(kind)
    rng = np.random.default_rng(4)
    args = batch_args(rng, B, kind)
    w = dev((rng.random(B) + 0.5).astype(np.float32))
    z = dev((1.5 * rng.normal(size=(B, 3 * N))).astype(np.float32))
    # head_values
    q, a, mq = T.head_values(z, dist)
    cq = torch.empty((B, 3), dtype=torch.float32, device=DEV)
    ca = torch.empty(B, dtype=torch.uint8, device=DEV)
    cm = torch.empty(B, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    assert L.qlx_head_values_dev(head.h, C.byref(dist.c), z.data_ptr(), B, cq.data_ptr(), ca.data_ptr(), cm.data_ptr()) == 0
    T.sync()
    assert same(host(q), host(cq)) and np.array_equal(host(a), host(ca)) and same(host(mq), host(cm))
    assert same(host(mq), host(q).max(axis=1)) and np.array_equal(host(a), host(q).argmax(axis=1))
    out = dict(actions=torch.zeros(B, dtype=torch.uint8, device=DEV))
    assert T.head_values(z, dist, want="actions", out=out) is out["actions"] and np.array_equal(host(out["actions"]), host(ca))
    # dist_loss
    loss, dz, sl, a_star = T.dist_loss(z, dist, *args, weights=w)
    assert not loss.requires_grad
    cb = qlx.DistBatch(*(t.data_ptr() for t in args), None, w.data_ptr())
    cdz, cl, csl = torch.empty_like(dz), torch.empty_like(loss), torch.empty_like(sl)
    cas = torch.empty_like(a_star)
    torch.cuda.synchronize()
    assert L.qlx_head_dist_loss_dev(head.h, C.byref(dist.c), z.data_ptr(), C.byref(cb), B, cdz.data_ptr(), cl.data_ptr(),
                                    csl.data_ptr(), cas.data_ptr()) == 0
    T.sync()
    assert same(host(dz), host(cdz)) and same(host(loss), host(cl)) and same(host(sl), host(csl))
    assert np.array_equal(host(a_star), host(cas))
    assert np.isfinite(host(loss)) and host(loss) > 0 and np.abs(host(dz)).max() > 0
    # the loss is the weighted mean of the sample losses (one rounding per operation of a sum of B terms)
    want = float((host(w).astype(np.float64) * host(sl).astype(np.float64)).mean())
    assert abs(float(host(loss)) - want) <= (B + 2) * 2.0 ** -24 * want
    T.close()


@pytest.mark.parametrize("kind", ["quantile", "categorical"])
def test_dist_loss_under_autograd_and_train_dist(world, kind):
    """three identically seeded nets take one update: (a) forward(head=True), 3 * dist_loss, backward(), step(); (b) the
    same by hand with backward_dz(3 * dz); (c) train_dist with weights 3.  (a) and (b) are the same bits; (c) scales inside
    the kernel (w g / B against 3 (g / B)), so its loss - a sum of 17 terms 3 L_b, six additions deep, against 3 times the sum of
    L_b - is compared within 16 roundings, and its update is checked to have happened."""
    B = 17
    dist = dist_of(kind)
    nets = [net(seed=5) for _ in range(3)]
    for T in nets:
        T.attach_head(3 * N, seed=8)
    A, H, F = nets
    src = source(world, B, 1)
    args = batch_args(np.random.default_rng(6), B, kind)
    # (a)
    _, z = A.forward(head=True, **src)
    loss, dz, sl, a_star = A.dist_loss(z, dist, *args)
    assert loss.requires_grad and not dz.requires_grad and not sl.requires_grad
    (3.0 * loss).backward()
    ga = [host(g) for g in A.grads()] + [host(g) for g in A.head_grads()]
    A.step()
    # (b)
    with torch.no_grad():
        _, zh = H.forward(head=True, **src)
        ticket = H.forward_ticket()
        loss_h, dz_h, _, _ = H.dist_loss(zh, dist, *args)
    assert same(host(zh), host(z)) and same(host(dz_h), host(dz)) and same(host(loss_h), host(loss))
    H.backward_dz(dz_h * 3.0, None, ticket, **src)
    gh = [host(g) for g in H.grads()] + [host(g) for g in H.head_grads()]
    H.step()
    for v, (x, y) in enumerate(zip(ga, gh)):
        assert same(x, y), v
    assert np.abs(ga[0]).max() > 0 and np.abs(ga[10]).max() > 0
    # (c)
    loss_f, sl_f = F.train_dist(dist, *args, weights=dev(np.full(B, 3, np.float32)), want_sample_loss=True, **src)
    assert same(host(sl_f), host(sl))
    assert abs(float(host(loss_f)) - 3 * float(host(loss))) <= 16 * 2.0 ** -24 * 3 * float(host(loss))
    none_loss, none_sl = F.train_dist(dist, *args, **src)
    assert none_sl is None and np.isfinite(host(none_loss))
    assert len(F._dist_work) == 1, "the work tensors are allocated once per width"
    for T in nets:
        T.sync()
    assert A.model.iterations() == H.model.iterations() == 1 and F.model.iterations() == 2
    assert A.head.iterations() == H.head.iterations() == 1 and F.head.iterations() == 2
    for which in range(3):
        for v in range(qlx.NUM_VARS):
            assert same(A.model.get(v, which), H.model.get(v, which)), (v, which)
        for var in range(2):
            assert same(A.head.get(var, which), H.head.get(var, which)), (var, which)
    for T in nets:
        T.close()


def test_misuse_raises(world):
    env, rb = world
    B = 4
    T = net()
    dist = QT.Quantile(N)
    args = batch_args(np.random.default_rng(2), B, "quantile")
    z = torch.zeros((B, 3 * N), device=DEV)
    with pytest.raises(RuntimeError, match="attach_head"):
        T.head_values(z, dist)
    with pytest.raises(RuntimeError, match="attach_head"):
        T.train_dist(dist, *args, **source(world, B))
    T.attach_head(3 * N)
    with pytest.raises(ValueError, match="atoms"):
        QT.Quantile(0)
    with pytest.raises(ValueError, match="atoms"):
        QT.Categorical(1, 0.0, 1.0)
    with pytest.raises(ValueError, match="v_min"):
        QT.Categorical(51, 1.0, 1.0)
    with pytest.raises(ValueError, match="width"):
        T.dist_loss(z, QT.Quantile(50), *args)
    with pytest.raises(ValueError, match="Quantile"):
        T.head_values(z, "quantile")
    with pytest.raises(ValueError, match="z_next"):
        T.dist_loss(z, dist, *args[:4], args[4][:, :5].contiguous())
    with pytest.raises(ValueError, match="actions"):
        T.train_dist(dist, args[0].to(torch.int64), *args[1:], **source(world, B))
    with pytest.raises(ValueError, match="want"):
        T.head_values(z, dist, want="nothing")
    assert T.model.iterations() == 0
    # one backward per step(), through the loss Function too
    src = source(world, B, 3)
    _, z1 = T.forward(head=True, **src)
    T.dist_loss(z1, dist, *args)[0].backward()
    _, z2 = T.forward(head=True, **src)
    with pytest.raises(RuntimeError, match="second backward"):
        T.dist_loss(z2, dist, *args)[0].backward()
    # train_dist overwrites the pending gradient, as train does
    T.train_dist(dist, *args, **src)
    _, z3 = T.forward(head=True, **src)
    T.dist_loss(z3, dist, *args)[0].backward()
    T.step()
    # an env stepped between the forward and the loss's backward: its states are read in place
    e2 = QT.TorchEnv(B, 7, DEV)
    _, z4 = T.forward(head=True, env=e2, layout=LAY)
    loss = T.dist_loss(z4, dist, *args)[0]
    e2.step(dev(np.zeros(B, np.uint8)))
    with pytest.raises(RuntimeError, match="stepped"):
        loss.backward()
    # ... and a replay pushed to
    rb2 = QT.TorchReplay(16, e2)
    a = dev(np.zeros(B, np.uint8))
    r, d = e2.step(a)
    rb2.add(e2, a, r, d)
    _, z5 = T.forward(head=True, replay=rb2, indices=dev(np.arange(B, dtype=np.int64)), layout=LAY)
    loss = T.dist_loss(z5, dist, *args)[0]
    r, d = e2.step(a)
    rb2.add(e2, a, r, d)
    with pytest.raises(RuntimeError, match="pushed"):
        loss.backward()
    T.sync()
    rb2.close(), e2.close(), T.close()


@pytest.mark.parametrize("flags", [[], ["--fused"], ["--c51", "--fused", "--per"]], ids=["torch", "fused", "c51-fused-per"])
def test_example_runs(flags):
    """20 updates at 16 envs: the script ends with a finite last loss"""
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "torch_qrdqn_example.py"), "--envs", "16", "--updates", "20",
           "--batch", "16", "--replay", "2000", "--warmup-steps", "4"] + flags
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    m = re.search(r"done \(([^)]*)\): 20 updates.*last loss ([-+0-9.eE]+|nan|inf)", done.stdout)
    assert m, done.stdout[-2000:]
    assert ("fused update" in m.group(1)) == ("--fused" in flags) and ("C51" in m.group(1)) == ("--c51" in flags)
    assert np.isfinite(float(m.group(2))) and float(m.group(2)) > 0
