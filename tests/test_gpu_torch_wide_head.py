"""The autograd path of the wide output head (qlx_torch.TorchQNet.attach_head, forward(head=True)) on the GPU.

A loss written in torch on (q, z) backpropagates through one autograd.Function with two outputs.  Two losses - the
quantile-Huber loss of QR-DQN on z alone, and a dueling loss that uses q and z together - are checked against a float64 torch
restatement of the dense part (Z = a4 Wh + bh, Q = a4 W4 + b4, a4 = relu(a3 W3 + b3) with the GPU's own ReLU decisions) fed the
GPU's a3 and a4 and the loss gradients autograd handed to the kernels, within the bounds of tests/test_gpu_wide_head.py
case 3; then the misuse errors, the bf16 refusal, copy_weights_from, and that every call without head=True on a net with a
head gives the bits of a net without one."""
import ctypes as C

import numpy as np
import pytest
import torch

import qlx_torch as QT   # before any other use of qlx in this process (it checks that itself)
import qlx

import wide_head_reference as R
from test_gpu_wide_head import DEV, LAY, a4_of, check, dev, grads_host, head_grads_host, host, net, same, source, world  # noqa: F401

pytestmark = pytest.mark.gpu

N_Q = 17   # quantiles per action: width 51, a ragged fourth tile


def a3_of(m, n):
    got = np.zeros((n, 3136), np.float32)
    assert qlx.lib().qlx_model_last_activation(m.h, 3, got.ctypes.data_as(C.c_void_p)) == 0
    return got


def quantile_huber(z, actions, target):
    """QR-DQN (Dabney et al. 2018, eq. 10) with kappa = 1: z [B, 3 N] quantiles per action, target [B, N]"""
    B = z.shape[0]
    n = z.shape[1] // 3
    theta = z.view(B, 3, n)[torch.arange(B, device=z.device), actions.long()]   # [B, N]
    u = target[:, None, :] - theta[:, :, None]                                   # [B, i, j]
    huber = torch.where(u.abs() <= 1, 0.5 * u * u, u.abs() - 0.5)
    tau = (torch.arange(n, device=z.device, dtype=z.dtype) + 0.5) / n
    return ((tau[None, :, None] - (u.detach() < 0).to(z.dtype)).abs() * huber).mean(dim=2).sum(dim=1).mean()


def dueling(q, z, actions, y):
    """Q = V + A - mean A from the head's 1 + 3 outputs, a Huber TD loss on it, and the plain head pulled towards it"""
    v, a = z[:, :1], z[:, 1:4]
    qd = v + a - a.mean(dim=1, keepdim=True)
    idx = actions.long()[:, None]
    td = torch.nn.functional.smooth_l1_loss(qd.gather(1, idx)[:, 0], y)
    return td + 0.25 * ((q - qd.detach()) ** 2).mean() + 0.1 * (q.gather(1, idx)[:, 0] - y).abs().mean()


def dense_restatement(a3, a4, w3, wh, bh, w4, b4, dz, dq):
    """float64 torch: the gradients of sum(dz * Z) + sum(dq * Q) w.r.t. Wh, bh, W4, b4, W3, b3, through
    a4 = mask * (a3 W3 + b3) with the GPU's mask a4 > 0"""
    t = lambda x: torch.tensor(np.asarray(x, np.float64))
    W3, Wh, bh_, W4, b4_ = (t(x).requires_grad_() for x in (w3, wh, bh, w4, b4))
    b3 = torch.zeros(512, dtype=torch.float64, requires_grad=True)
    pre = t(a3) @ W3 + b3
    x4 = t(a4) + t((a4 > 0).astype(np.float64)) * (pre - pre.detach())   # the GPU's a4 as the value, the mask as the slope
    loss = ((x4 @ Wh + bh_) * t(dz)).sum()
    if dq is not None:
        loss = loss + ((x4 @ W4 + b4_) * t(dq)).sum()
    loss.backward()
    g = lambda p: p.grad.numpy() if p.grad is not None else np.zeros(tuple(p.shape))
    return dict(dwh=g(Wh), dbh=g(bh_), dw4=g(W4), db4=g(b4_), dw3=g(W3), db3=g(b3))


@pytest.mark.parametrize("which", ["quantile", "dueling"])
def test_autograd_against_the_float64_dense_restatement(world, which):
    B = 33
    width = 3 * N_Q if which == "quantile" else 4
    T = net()
    head = T.attach_head(width, seed=12)
    rng = np.random.default_rng(width)
    src = source(world, B, 40 + width)
    actions = dev(rng.integers(0, 3, B).astype(np.uint8))
    q, z = T.forward(head=True, **src)
    assert q.requires_grad and z.requires_grad and tuple(z.shape) == (B, width) and tuple(q.shape) == (B, 3)
    q.retain_grad()
    z.retain_grad()
    if which == "quantile":
        target = dev((rng.normal(size=(B, N_Q)) * 2).astype(np.float32)) + z.detach().mean()
        loss = quantile_huber(z, actions, target)
    else:
        y = dev(rng.normal(size=B).astype(np.float32)) + q.detach().mean()
        loss = dueling(q, z, actions, y)
    ticket = T.forward_ticket()
    loss.backward()
    assert T.forward_ticket() == ticket, "the backward ran a forward of its own"
    dz = host(z.grad)
    dq = None if q.grad is None else host(q.grad)
    assert (dq is None) == (which == "quantile"), "a loss of z alone passes no dq"
    assert np.abs(dz).max() > 0
    a3, a4 = a3_of(T.model, B), a4_of(T.model, B)
    # the loss gradient itself against float64 torch on the same outputs (fp32 torch arithmetic: 1e-5 of its largest)
    z64 = torch.tensor(host(z.detach()).astype(np.float64), requires_grad=True)
    q64 = torch.tensor(host(q.detach()).astype(np.float64), requires_grad=True)
    if which == "quantile":
        quantile_huber(z64, actions.cpu(), target.cpu().double()).backward()
    else:
        dueling(q64, z64, actions.cpu(), y.cpu().double()).backward()
    assert np.abs(dz - z64.grad.numpy()).max() <= 1e-5 * np.abs(dz).max()
    if dq is not None:
        assert np.abs(dq - q64.grad.numpy()).max() <= 1e-5 * np.abs(dq).max()
    # the kernels' gradients against the dense restatement, within case 3's bounds
    wh, bh = head.get(0), head.get(1)
    w3, w4, b4 = T.model.get(6), T.model.get(8), T.model.get(9)
    ref = dense_restatement(a3, a4, w3, wh, bh, w4, b4, dz, dq)
    g, (dwh, dbh) = grads_host(T), head_grads_host(T)
    print(f"{which}: width {width}, B {B}")
    _, _, tw, tb = R.weight_grads(a4, dz)
    check("dWh", dwh, ref["dwh"], R.gamma(B + 1) * tw)
    check("dbh", dbh, ref["dbh"], R.gamma(B + 1) * tb)
    d4, t4 = R.backward_data(a4, wh, dz, w4, dq)
    coeff = R.gamma(width + 3) + R.gamma(B)   # dz4's chain, then the sum over the batch
    assert np.abs(ref["db3"] - d4.sum(axis=0)).max() <= 1e-12 * (1 + np.abs(d4).max() * B), "the two restatements disagree"
    check("db3", g[7], ref["db3"], coeff * t4.sum(axis=0))
    check("dW3", g[6], ref["dw3"], coeff * (np.abs(a3.astype(np.float64)).T @ t4))
    if dq is not None:
        _, _, t4w, t4b = R.weight_grads(a4, dq)
        check("dW4", g[8], ref["dw4"], R.gamma(B + 1) * t4w)
        check("db4", g[9], ref["db4"], R.gamma(B + 1) * t4b)
    else:
        assert not g[8].any() and not g[9].any()
    # step() steps both
    w_before, wh_before = T.model.get(6), head.get(0)
    T.step()
    T.sync()
    assert T.model.iterations() == 1 and head.iterations() == 1
    assert not same(T.model.get(6), w_before) and not same(head.get(0), wh_before)
    T.close()


def test_misuse_raises(world):
    env, rb = world
    B = 4
    T = net()
    src = source(world, B, 3)
    with pytest.raises(RuntimeError, match="attach_head"):
        T.forward(head=True, **src)
    with pytest.raises(RuntimeError, match="attach_head"):
        T.head_grads()
    T.attach_head(8)
    # one backward per step()
    q, z = T.forward(head=True, **src)
    z.sum().backward()
    q2, z2 = T.forward(head=True, **src)
    with pytest.raises(RuntimeError, match="second backward"):
        (z2.sum() + q2.sum()).backward()
    T.step()
    # an env stepped between forward and backward
    e2 = QT.TorchEnv(B, 7, DEV)
    q, z = T.forward(head=True, env=e2, layout=LAY)
    e2.step(dev(np.zeros(B, np.uint8)))
    with pytest.raises(RuntimeError, match="stepped"):
        z.sum().backward()
    # ... and a replay pushed to
    rb2 = QT.TorchReplay(16, e2)
    a = dev(np.zeros(B, np.uint8))
    r, d = e2.step(a)
    rb2.add(e2, a, r, d)
    q, z = T.forward(head=True, replay=rb2, indices=dev(np.arange(B, dtype=np.int64)), layout=LAY)
    r, d = e2.step(a)
    rb2.add(e2, a, r, d)
    with pytest.raises(RuntimeError, match="pushed"):
        q.sum().backward()
    # no_grad: the plain forward, up to the reserve, for acting on an env ring
    with torch.no_grad():
        q, z = T.forward(head=True, env=e2, layout=LAY)
    assert not q.requires_grad and not z.requires_grad and tuple(z.shape) == (B, 8)
    # wrong shapes are refused before anything is launched
    with pytest.raises(ValueError, match="dz"):
        T.backward_dz(torch.zeros((B, 7), device=DEV), None, 0, **src)
    T.sync()
    rb2.close(), e2.close(), T.close()


def test_bf16_net_takes_no_head():
    T = net(arch="bf16", reserve=8)
    with pytest.raises(qlx.QlError):
        T.attach_head(4)
    assert T.head is None
    T.close()


def test_copy_weights_from_copies_the_head(world):
    A, T, P = net(seed=5), net(seed=6), net(seed=7)
    ha, ht = A.attach_head(20, seed=1), T.attach_head(20, seed=2)
    ha.set(1, np.arange(20, dtype=np.float32))
    ha.set(0, ha.get(0) * 2, which=1)   # Adam slots are not part of the copy
    assert not same(ha.get(0), ht.get(0))
    T.copy_weights_from(A)
    T.sync()
    assert same(ht.get(0), ha.get(0)) and same(ht.get(1), ha.get(1))
    assert not ht.get(0, 1).any()
    for v in range(qlx.NUM_VARS):
        assert same(T.model.get(v), A.model.get(v))
    # a net without a head takes the ten variables only; heads of different widths are refused
    P.copy_weights_from(A)
    P.sync()
    assert same(P.model.get(8), A.model.get(8))
    P.attach_head(21)
    with pytest.raises(ValueError, match="widths"):
        P.copy_weights_from(A)
    assert qlx.lib().qlx_head_copy_weights_dev(P.head.h, ha.h) == -1
    # the copy is seen by the next forward
    src = source(world, 5, 9)
    with torch.no_grad():
        _, za = A.forward(head=True, **src)
        _, zt = T.forward(head=True, **src)
    assert same(host(za), host(zt))
    A.close(), T.close(), P.close()


def test_calls_without_the_head_are_unchanged(world):
    """a net with a head, used without head=True, against a net without one: the same bits from q, forward / backward /
    step, train and copy_weights_from"""
    B = 17
    A, T = net(), net()
    head = T.attach_head(29, seed=8)
    wh0 = head.get(0)
    src = source(world, B, 5)
    rng = np.random.default_rng(5)
    for m in (A, T):
        m.results = []
        qv, act, mx = m.q(**src)
        m.results += [host(qv), host(act).astype(np.float32), host(mx)]
        q = m(**src)
        ((q - 1.0) ** 2).mean().backward()
        m.results += grads_host(m)
        m.step()
        loss, td = m.train(dev(np.arange(B, dtype=np.uint8) % 3), dev(np.ones(B, np.float32)), want_td_abs=True, **src)
        m.results += [host(loss).reshape(1), host(td)] + grads_host(m)
        m.step()
        m.sync()
        m.results += [m.model.get(v, which) for v in range(qlx.NUM_VARS) for which in range(3)]
    assert len(A.results) == len(T.results)
    for i, (a, b) in enumerate(zip(A.results, T.results)):
        assert same(a, b), i
    assert A.model.iterations() == T.model.iterations() == 3
    assert head.iterations() == 0 and same(head.get(0), wh0)
    A.close(), T.close()
