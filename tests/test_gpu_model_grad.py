"""A caller's own loss through the Q-net's HIP kernels on the GPU (include/qlx.h "a caller's own loss"):
qlx_model_backward_dev / qlx_model_step_dev / qlx_model_grads_dev and the autograd path of qlx_torch.TorchQNet.

1. Exact anchor: a dq that is the training head's own dloss/dq (restated in numpy float32) at the taken action and zero
   elsewhere gives the gradient buffer, and after step() the weights, Adam slots and iteration count, of the built-in update
   on a twin model - as bytes, both archs, all three state sources.
2. A backward that reuses its forward's activations (the ticket), one that recomputes (ticket 0) and one whose ticket went
   stale give the same bytes.
3. A dense dq (all three actions) against references that do not share the kernels' arithmetic: fp32 against the float64
   torch restatement of tests/test_oracle_qnet32_pin.py with the GPU's own ReLU decisions (bound: that file's 1e-4 of the
   variable's largest gradient), bf16 block-wise against the forced emulation of tests/bf16_reference.py (bound:
   tests/bf16_checks.py BLOCK_REL).  The one-hot case is measured the same way and printed beside it.
4. step(grads_written=True) after scaling the buffer by 0.5 equals qlx_model_apply_gradient(grads, 0.5) on a twin; a step
   before any gradient is refused.
5. The torch layer: net(obs) -> torch's Huber -> backward() -> step() against train() (fp32; torch's Huber gradient may
   round differently from the head's, so: gradients within 1e-4, weights within 1e-7 + 1e-6 max|w|), the misuse errors,
   the shapes of grads(), no_grad.
All comparisons are made on bytes copied back to the host."""
import ctypes as C

import numpy as np
import pytest
import torch

import qlx_torch as QT   # before any other use of qlx in this process (it checks that itself)
import qlx

import bf16_checks
import bf16_reference
from test_oracle_qnet32_pin import relmax, torch_forward

pytestmark = pytest.mark.gpu

SEED = 0x51A5EED
DEV = "cuda:0"
ARCHS = ["f32", "bf16"]
PER_SAMPLE = (12800, 5184, 3136, 512)
ACT_SHAPES = ((20, 20, 32), (9, 9, 64), (7, 7, 64), (512,))
LAY = "nhwc_slot"   # the convention of the host calls and of both references


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def host(t):
    return t.cpu().numpy()


def dev(a):
    return torch.as_tensor(np.array(a, order="C")).to(DEV)


def net(arch, seed=5, reserve=64, env=None):
    return QT.TorchQNet(arch, seed=seed, device=DEV, env=env, reserve=reserve)


def model_state(model):
    return [model.get(v, w) for v in range(qlx.NUM_VARS) for w in range(3)], model.iterations()


def same_state(a, b):
    return a[1] == b[1] and all(same(x, y) for x, y in zip(a[0], b[0]))


def grads_host(m):
    return [host(g) for g in m.grads()]


def activations(m, n):
    out = []
    for layer in range(1, 5):
        got = np.zeros(n * PER_SAMPLE[layer - 1], np.float32)
        assert qlx.lib().qlx_model_last_activation(m.h, layer, got.ctypes.data_as(C.c_void_p)) == 0
        out.append(got.reshape((n,) + ACT_SHAPES[layer - 1]))
    return out


def head_dq(q, a, y, w):
    """dloss/dq of the training head (k_head32<3> / k_fc2_train), one rounded float32 operation per step: e = q_a - y,
    ge = e inside the Huber knee and its sign outside, (w * ge) / B at the taken action, zero elsewhere"""
    f = np.float32
    B = len(a)
    e = (q[np.arange(B), a] - y).astype(f)
    ge = np.where(np.abs(e) <= f(1.0), e, np.sign(e)).astype(f)
    g = ((w * ge).astype(f) / f(B)).astype(f)
    dq = np.zeros((B, 3), f)
    dq[np.arange(B), a] = g
    assert e.dtype == ge.dtype == g.dtype == f
    return dq


def head_inputs(q, rng):
    """actions, targets on both sides of the Huber knee, random per-sample weights"""
    B = len(q)
    a = rng.integers(0, 3, B).astype(np.uint8)
    y = (q[np.arange(B), a] + rng.choice([-2.5, -0.4, 0.3, 1.7], size=B)).astype(np.float32)
    w = rng.uniform(0.25, 1.5, B).astype(np.float32)
    return a, y, w


@pytest.fixture(scope="module")
def pool():
    """520 real env states six steps into play; every fourth env was reset after the third step, so its older channels
    are zero frames and the ring phases differ"""
    n = 520
    te = QT.TorchEnv(n, SEED, DEV)
    rng = np.random.default_rng(5)
    for t in range(6):
        te.step(dev(rng.integers(0, 3, n).astype(np.uint8)))
        if t == 2:
            te.reset(dev((np.arange(n) % 4 == 1).astype(np.uint8)))
    te.sync()
    x = te._env.state().copy()
    te.close()
    assert x.shape == (n, 84, 84, 4) and x[0].any()
    assert any(not x[i, :, :, c].any() for i in (1, 5) for c in range(4)), "no zero frame"
    x.setflags(write=False)
    return x


# ---------------------------------------------------------------- 1. the exact anchor

def anchor(A, T, src, B, rng, steps=2):
    """`steps` updates of A by forward / backward(dq of the head) / step and of its twin T by train(): the same bytes"""
    for step in range(1, steps + 1):
        q = host(A.q(want="q", layout=LAY, **src))
        ticket = A.forward_ticket()
        a, y, w = head_inputs(q, rng)
        A.backward_dq(dev(head_dq(q, a, y, w)), ticket, layout=LAY, **src)
        assert A.forward_ticket() == ticket, "the backward ran a forward of its own"
        T.train(dev(a), dev(y), dev(w), layout=LAY, **src)
        gA, gT = grads_host(A), grads_host(T)
        for v in range(qlx.NUM_VARS):
            assert gA[v].shape == tuple(qlx.VAR_SHAPES[v])
            assert same(gA[v], gT[v]), (step, v, float(np.abs(gA[v] - gT[v]).max()), float(np.abs(gT[v]).max()))
        assert A.model.iterations() == step - 1
        A.step()
        A.sync(), T.sync()
        assert same_state(model_state(A.model), model_state(T.model)), step


# 3 and 17: ragged head blocks (4 samples per block in both backends); 33: more than one 16-sample fragment; 513: crosses
# SideFc2's 512-sample LDS pass, the bf16 dense-3 blocks' 512-thread stride and their GEMMs' 128-row tiles
@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("B", [1, 3, 17, 33, 513])
def test_one_hot_dq_is_the_training_head(pool, arch, B):
    A, T = net(arch, reserve=B), net(arch, reserve=B)
    anchor(A, T, dict(obs=dev(pool[:B])), B, np.random.default_rng(B))
    A.close(), T.close()


N_ENVS, CAP, STEPS = 3, 37, 20


@pytest.fixture(scope="module")
def world():
    """3 envs, capacity 37, 20 vector steps = 60 pushes: the ring has wrapped; resets leave zero frames"""
    env = QT.TorchEnv(N_ENVS, SEED, DEV)
    rb = QT.TorchReplay(CAP, env)
    rng = np.random.default_rng(17)
    for t in range(STEPS):
        a = dev(rng.integers(0, 3, N_ENVS).astype(np.uint8))
        r, d = env.step(a)
        rb.add(env, a, r, d)
        if t in (9, 12):
            env.reset(dev(np.array([t == 9, t == 12, 0], np.uint8)))
    rb.sync()
    assert len(rb) == CAP
    return env, rb


@pytest.mark.parametrize("arch", ARCHS)
def test_one_hot_dq_from_replay_and_env(world, arch):
    env, rb = world
    B = 17
    idx = dev((np.arange(B, dtype=np.int64) * 7 + 3) % CAP)
    A, T = net(arch), net(arch)
    anchor(A, T, dict(replay=rb, indices=idx), B, np.random.default_rng(1), steps=1)
    A.close(), T.close()
    A, T = net(arch), net(arch)
    anchor(A, T, dict(env=env), N_ENVS, np.random.default_rng(2), steps=1)
    A.close(), T.close()
    rb.sync()


# ---------------------------------------------------------------- 2. reuse = recompute

@pytest.mark.parametrize("arch", ARCHS)
def test_reuse_equals_recompute(pool, arch):
    B = 33
    A = net(arch, reserve=64)
    x, other = dev(pool[:B]), dev(pool[100:100 + 40])
    dq = dev(np.random.default_rng(3).standard_normal((B, 3)).astype(np.float32))
    A.q(x, layout=LAY, want="q")
    t0 = A.forward_ticket()
    assert t0 != 0
    A.backward_dq(dq, t0, x, layout=LAY)
    assert A.forward_ticket() == t0
    reused = grads_host(A)
    assert any(g.any() for g in reused)
    A.backward_dq(dq, 0, x, layout=LAY)
    assert A.forward_ticket() != t0, "ticket 0 runs the forward again"
    recomputed = grads_host(A)
    A.q(x, layout=LAY, want="q")
    t1 = A.forward_ticket()
    A.q(other, layout=LAY, want="actions")   # another batch size, other states: t1 is stale
    assert A.forward_ticket() != t1
    A.backward_dq(dq, t1, x, layout=LAY)
    stale = grads_host(A)
    for v in range(qlx.NUM_VARS):
        assert same(reused[v], recomputed[v]) and same(reused[v], stale[v]), v
    A.sync()
    A.close()


# ---------------------------------------------------------------- 3. a dense dq against independent references

def f64_reference(m, x, dq):
    """float64 torch gradients of (q * dq).sum() with the GPU's ReLU decisions, each unit where they differ from float64
    torch's own checked to sit at the kink (the method of tests/test_oracle_qnet32_pin.py kink_masks)"""
    ws = m.model.weights()
    acts = activations(m, len(x))
    _, _, pre, _ = torch_forward(ws, x)
    masks = []
    for l in range(4):
        mask = acts[l] > 0
        diff = mask != (pre[l] > 0)
        assert np.all(np.abs(pre[l][diff]) <= 1e-5 * np.abs(pre[l]).max()), f"layer {l + 1}: mask differs off the kink"
        masks.append(mask)
    q, _, _, params = torch_forward(ws, x, masks)
    (q * torch.as_tensor(dq.astype(np.float64))).sum().backward()
    return [p.grad.numpy() for p in params]


def bf16_forced_reference(weights, x, acts, dq):
    """tests/bf16_reference.py forward_backward_full's forced emulation with the caller's dq in place of its head: the
    product's stored a1 .. a4, dz4 = bf16(the float32 fmaf chain over n of W4[k][n] dq[b][n]) (a4 > 0)"""
    R = bf16_reference
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
    ws = [t(w) for w in weights]
    for i in (0, 2, 4, 6):
        ws[i] = R.bf16(ws[i])
    params = [w.clone().requires_grad_(True) for w in ws]
    k0, b0, k1, b1, k2, b2, k3, b3, k4, b4 = params
    B = len(x)
    given = [t(a) for a in acts]
    nchw = lambda a: a.permute(0, 3, 1, 2)
    h = nchw(t(x))
    for l, (k, b, stride) in enumerate(((k0, b0, 4), (k1, b1, 2), (k2, b2, 1))):
        h = R._Forced.apply(torch.nn.functional.conv2d(h, k.permute(3, 2, 0, 1), b, stride=stride), nchw(given[l]))
    z4 = h.permute(0, 2, 3, 1).reshape(B, -1) @ k3 + b3
    q = given[3] @ k4 + b4
    f = np.float32
    w4, d = np.asarray(weights[8], f), np.asarray(dq, f)
    chain = (w4[None, :, 0] * d[:, None, 0]).astype(f)   # the first product is rounded
    for n in (1, 2):                                      # fmaf: the product is exact in float64
        chain = (w4[None, :, n].astype(np.float64) * d[:, None, n] + chain).astype(f)
    torch.autograd.backward([q, z4], [t(dq), R.bf16(t(chain)) * (given[3] > 0)])
    return [p.grad.numpy() for p in params]


def measure(arch, m, x, dq):
    """{variable: error} of the gradient buffer after a backward of dq, by the arch's own measure"""
    xd = dev(x)
    m.q(xd, layout=LAY, want="q")
    ticket = m.forward_ticket()
    if arch == "f32":
        ref = f64_reference(m, x, dq)
    else:
        ref = bf16_forced_reference(m.model.weights(), x, activations(m, len(x)), dq)
    m.backward_dq(dev(dq), ticket, xd, layout=LAY)
    got = grads_host(m)
    if arch == "f32":
        return {v: relmax(got[v], ref[v]) for v in range(10)}
    return {v: max(err for _, err in bf16_checks.block_errors(got[v], ref[v], v)) for v in range(10)}


@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("B", [4, 33])
def test_dense_dq_against_reference(pool, arch, B):
    rng = np.random.default_rng(40 + B)
    x = np.ascontiguousarray(pool[8:8 + B])
    m = net(arch, seed=7)
    if arch == "bf16":
        m.model.set_weights(bf16_checks.nonzero_biases(m.model.weights(), 100 + B))
    bound = 1e-4 if arch == "f32" else bf16_checks.BLOCK_REL
    # all three actions non-zero, random signs, magnitudes over two decades around the head's 1 / B
    dense = (rng.choice([-1.0, 1.0], (B, 3)) * 10.0 ** rng.uniform(-1.5, 0.5, (B, 3)) / B).astype(np.float32)
    assert (dense != 0).all()
    q = host(m.q(dev(x), layout=LAY, want="q"))
    one_hot = head_dq(q, *head_inputs(q, rng))
    err_hot = measure(arch, m, x, one_hot)
    err_dense = measure(arch, m, x, dense)
    for v in range(10):
        print(f"{arch} B={B} var{v}: dense dq {err_dense[v]:.2e}, one-hot dq {err_hot[v]:.2e} (bound {bound:.1e})")
    for v in range(10):
        assert err_dense[v] <= bound, (v, err_dense[v], err_hot[v])
        assert err_hot[v] <= bound, (v, err_hot[v])
    m.close()


# ---------------------------------------------------------------- 4. step

@pytest.mark.parametrize("arch", ARCHS)
def test_step_on_a_written_buffer_is_apply_gradient(pool, arch):
    B = 17
    A, T = net(arch), net(arch)
    with pytest.raises(qlx.QlError, match="gradient"):
        A.step()
    assert A.model.iterations() == 0
    x = dev(pool[:B])
    dq = dev(np.random.default_rng(9).standard_normal((B, 3)).astype(np.float32) / B)
    A.q(x, layout=LAY, want="q")
    A.backward_dq(dq, A.forward_ticket(), x, layout=LAY)
    raw = np.concatenate([g.ravel() for g in grads_host(A)])
    for g in A.grads():
        g.mul_(0.5)
    A.step(grads_written=True)
    A.sync()
    T.model.apply_gradient(raw, 0.5)
    assert A.model.iterations() == 1
    assert same_state(model_state(A.model), model_state(T.model))
    A.close(), T.close()


# ---------------------------------------------------------------- 5. the torch layer

def test_torch_huber_through_autograd_matches_train(pool):
    B = 33
    A, T = net("f32"), net("f32")
    x = dev(pool[:B])
    rng = np.random.default_rng(21)
    for step in (1, 2):
        q = A(x, layout=LAY)
        assert q.grad_fn is not None and q.shape == (B, 3) and q.dtype == torch.float32
        a, y, _ = head_inputs(host(q.detach()), rng)
        qa = q[torch.arange(B, device=DEV), dev(a.astype(np.int64))]
        loss = torch.nn.functional.huber_loss(qa, dev(y), delta=1.0, reduction="mean")
        loss.backward()
        loss_ref, _ = T.train(dev(a), dev(y), obs=x, layout=LAY)
        assert abs(loss.item() - loss_ref.item()) <= 1e-5 * abs(loss_ref.item())
        gA, gT = grads_host(A), grads_host(T)
        for v in range(10):
            assert relmax(gA[v], gT[v].astype(np.float64)) <= 1e-4, (step, v)
        A.step()
        A.sync(), T.sync()
        assert A.model.iterations() == T.model.iterations() == step
        for v in range(10):
            w, wt = A.model.get(v), T.model.get(v)
            assert np.abs(w - wt).max() <= 1e-7 + 1e-6 * np.abs(wt).max(), (step, v)
    A.close(), T.close()


def test_torch_layer_misuse_and_shapes(pool, world):
    env, rb = world
    m = net("f32")
    x = dev(pool[:4])
    with torch.no_grad():
        q = m(x, layout=LAY)
    assert q.grad_fn is None and not q.requires_grad
    assert same(host(q), host(m.q(x, layout=LAY, want="q")))
    views = m.grads()
    assert [tuple(g.shape) for g in views] == [tuple(s) for s in qlx.VAR_SHAPES]
    assert all(g.dtype == torch.float32 and g.device == torch.device(DEV) for g in views)
    assert views[1].data_ptr() == views[0].data_ptr() + 4 * 8 * 8 * 4 * 32, "views of one flat buffer"

    # a second backward before step() / discard_grad()
    q1, q2 = m(x, layout=LAY), m(x, layout=LAY)
    q1.sum().backward()
    with pytest.raises(RuntimeError, match="second backward"):
        q2.sum().backward()
    m.discard_grad()
    m(x, layout=LAY).sum().backward()
    m.step()
    assert m.model.iterations() == 1

    # the env or the replay a forward read was written to before its backward
    qe = m(env=env, layout=LAY)
    env.step(dev(np.zeros(N_ENVS, np.uint8)))
    with pytest.raises(RuntimeError, match="TorchEnv"):
        qe.sum().backward()
    idx = dev(np.arange(5, dtype=np.int64))
    qr = m(replay=rb, indices=idx, layout=LAY)
    a = dev(np.zeros(N_ENVS, np.uint8))
    r, d = env.step(a)
    rb.add(env, a, r, d)
    with pytest.raises(RuntimeError, match="TorchReplay"):
        qr.sum().backward()
    assert m.model.iterations() == 1   # none of the refused backwards launched or left anything to step
    m(replay=rb, indices=idx, layout=LAY).sum().backward()   # untouched since its forward: fine
    m.step()
    m.sync(), rb.sync(), env.sync()
    m.close()
