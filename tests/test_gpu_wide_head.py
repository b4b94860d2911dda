"""The wide output head on the GPU (include/qlx.h "a wide output head"; csrc/head_wide.hip): qlx_head_* driven
through qlx.WideHead and the device-tensor plumbing of qlx_torch.TorchQNet (forward(head=True) under no_grad, backward_dz,
head_grads, step).  States are replay transitions of a TorchEnv stepped 30 times, so the conv skips see real frames.

1. Width-3 pin: a head holding W4 and b4 gives the model's own Q, gradients and update, bit for bit.
2. Column and batch invariance, and run-to-run identity, bit for bit.
3. Forward, weight gradients and backward data against the float64 restatement (tests/wide_head_reference.py) within the
   standard bound gamma(n) * sum |terms| per output, at widths 1, 16, 17, 153, 600, 1024 and batches 1, 5, 100.
4. clip_by_norm + Adam at those widths against the restatement fed the GPU's own raw gradients.
6. State errors.
(5, the autograd path, is tests/test_gpu_torch_wide_head.py.)  All comparisons are made on bytes copied back to the host;
"the same bits" compares the 32-bit patterns."""
import ctypes as C

import numpy as np
import pytest
import torch

import qlx_torch as QT   # before any other use of qlx in this process (it checks that itself)
import qlx

import wide_head_reference as R

pytestmark = pytest.mark.gpu

SEED = 0x51A5EED
DEV = "cuda:0"
LAY = "nchw_time"
N_ENVS, CAP, STEPS = 4, 128, 30
WIDTHS = [1, 16, 17, 153, 600, 1024]   # one column; one tile; a ragged second tile; ragged slabs of the data and weight
BATCHES = [1, 5, 100]                  # kernels (128 j, 64 columns); the largest width.  Batches: ragged 16-sample blocks


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def host(t):
    return t.cpu().numpy()


def dev(a):
    return torch.as_tensor(np.array(a, order="C")).to(DEV)


def net(seed=5, reserve=128, arch="f32"):
    return QT.TorchQNet(arch, seed=seed, device=DEV, reserve=reserve)


def grads_host(m):
    return [host(g) for g in m.grads()]


def head_grads_host(m):
    return [host(g) for g in m.head_grads()]


def a4_of(m, n):
    """a4 of the model's last forward (qlx_model_last_activation, layer 4)"""
    got = np.zeros((n, 512), np.float32)
    assert qlx.lib().qlx_model_last_activation(m.h, 4, got.ctypes.data_as(C.c_void_p)) == 0
    return got


@pytest.fixture(scope="module")
def world():
    """4 envs, 30 vector steps into a replay of 128: 120 transitions of play, two envs reset on the way"""
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
    assert len(rb) == N_ENVS * STEPS
    yield env, rb
    rb.close()
    env.close()


def source(world, B, seed=0):
    """B distinct transitions as a replay source; the first one is fixed, so that a sample can be found in two batches
    (transition 77: well into play - the state before an episode's first step is four zero frames, and Q of it is 0)"""
    _, rb = world
    rng = np.random.default_rng(1000 + seed)
    rest = rng.permutation(np.delete(np.arange(len(rb)), 77))[:B - 1]
    idx = np.concatenate([[77], rest]).astype(np.int64)
    return dict(replay=rb, indices=dev(idx), layout=LAY)


def forward_both(m, src):
    """(q, z, ticket) of a net with a head, no autograd"""
    with torch.no_grad():
        q, z = m.forward(head=True, **src)
    return host(q), host(z), m.forward_ticket()


# ---------------------------------------------------------------- 1. the width-3 pin

@pytest.mark.parametrize("B", [1, 3, 17, 100])
def test_width_3_head_is_the_models_own_head(world, B):
    A, T = net(), net()
    head = T.attach_head(3, seed=9)
    w4, b4 = A.model.get(8), A.model.get(9)
    head.set(0, w4)
    head.set(1, b4)
    src = source(world, B, B)
    rng = np.random.default_rng(B)
    qA = host(A.q(want="q", **src))
    tA = A.forward_ticket()
    qT, z, tT = forward_both(T, src)
    assert same(qT, qA) and same(z, qA)
    assert np.abs(qA).max() > 0
    dq = rng.normal(size=(B, 3)).astype(np.float32)
    A.backward_dq(dev(dq), tA, **src)
    T.backward_dz(dev(dq), None, tT, **src)
    assert A.forward_ticket() == tA and T.forward_ticket() == tT, "a backward ran a forward of its own"
    gA, gT, gH = grads_host(A), grads_host(T), head_grads_host(T)
    for v in range(8):
        assert same(gA[v], gT[v]), (v, float(np.abs(gA[v] - gT[v]).max()))
        assert np.abs(gA[v]).max() > 0, v
    assert same(gH[0], gA[8]) and same(gH[1], gA[9])
    assert not gT[8].any() and not gT[9].any(), "dW4 / db4 of a backward without dq"
    A.step()
    T.step()
    A.sync(), T.sync()
    assert head.iterations() == 1 and A.model.iterations() == 1 and T.model.iterations() == 1
    for which in range(3):
        assert same(head.get(0, which), A.model.get(8, which)), which
        assert same(head.get(1, which), A.model.get(9, which)), which
        for v in range(8):
            assert same(T.model.get(v, which), A.model.get(v, which)), (v, which)
    assert same(T.model.get(8), w4) and same(T.model.get(9), b4), "W4 / b4 moved under a zero gradient"
    assert not same(head.get(0), w4), "the head did not move"
    A.close(), T.close()


# ---------------------------------------------------------------- 2. invariance

def test_columns_and_batches_do_not_see_each_other(world):
    B = 100
    A, T = net(), net()
    head = T.attach_head(37, seed=4)
    wh, bh = head.get(0), head.get(1) + np.float32(0.25)
    wh[:, 17:20], bh[17:20] = A.model.get(8), A.model.get(9)
    head.set(0, wh)
    head.set(1, bh)
    src = source(world, B, 2)
    qA = host(A.q(want="q", **src))
    tA = A.forward_ticket()
    qT, z, tT = forward_both(T, src)
    assert same(z[:, 17:20], qA) and same(qT, qA)
    assert np.abs(z[:, :17]).max() > 0 and np.abs(z[:, 20:]).max() > 0
    # a dz that is non-zero only in those columns: the trunk gradient of the model's own head with that dq
    dq = np.random.default_rng(2).normal(size=(B, 3)).astype(np.float32)
    dz = np.zeros((B, 37), np.float32)
    dz[:, 17:20] = dq
    A.backward_dq(dev(dq), tA, **src)
    T.backward_dz(dev(dz), None, tT, **src)
    gA, gT, gH = grads_host(A), grads_host(T), head_grads_host(T)
    for v in range(8):
        assert same(gA[v], gT[v]), v
    assert same(gH[0][:, 17:20], gA[8]) and same(gH[1][17:20], gA[9])
    assert not gH[0][:, :17].any() and not gH[0][:, 20:].any()
    # sample 0 alone and inside the batch of 100
    one = dict(src, indices=src["indices"][:1].clone())
    _, z1, _ = forward_both(T, one)
    assert same(z1[0], z[0])
    # a second run: identical bits everywhere
    T.discard_grad()
    _, z2, t2 = forward_both(T, src)
    T.backward_dz(dev(dz), None, t2, **src)
    assert same(z2, z)
    for a, b in zip(grads_host(T) + head_grads_host(T), gT + gH):
        assert same(a, b)
    A.close(), T.close()


# ---------------------------------------------------------------- 3. the float64 restatement

def check(name, got, ref, bound):
    err = np.abs(np.asarray(got, np.float64) - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"  {name}: max err / bound = {worst:.3g}, max |ref| = {float(np.abs(ref).max()):.3g}")
    assert (err <= bound).all(), (name, worst)
    assert np.isfinite(got).all() and np.abs(ref).max() > 0, name


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("width", WIDTHS)
def test_against_the_float64_restatement(world, width, B):
    """Bounds (derived, not measured; u = 2^-24, gamma(n) = n u / (1 - n u)), each times the sum of the absolute terms of
    the output's chain: Z gamma(520) (512 products in four chains, three adds, the bias); dWh, dbh gamma(B + 1); dz4, seen
    as db3 = sum over b of dz4[b] (variable 7; the row itself at B = 1), gamma(width + 3), plus gamma(B) for that sum."""
    T = net()
    head = T.attach_head(width, seed=width)
    rng = np.random.default_rng(31 * width + B)
    head.set(1, rng.normal(size=width).astype(np.float32))
    wh, bh, w4 = head.get(0), head.get(1), T.model.get(8)
    assert np.abs(wh).max() <= np.sqrt(6.0 / (512 + width)) and np.abs(wh).max() > 0.5 * np.sqrt(6.0 / (512 + width))
    src = source(world, B, width)
    _, z, ticket = forward_both(T, src)
    a4 = a4_of(T.model, B)
    assert (a4 > 0).any() and (a4 == 0).any()
    print(f"width {width}, B {B}")
    zr, zt = R.forward(a4, wh, bh)
    check("Z", z, zr, R.gamma(520) * zt)
    dz = rng.normal(size=(B, width)).astype(np.float32)
    dq = rng.normal(size=(B, 3)).astype(np.float32)
    for with_dq in (False, True):
        T.backward_dz(dev(dz), dev(dq) if with_dq else None, ticket, **src)
        g, (dwh, dbh) = grads_host(T), head_grads_host(T)
        T.discard_grad()
        rw, rb, tw, tb = R.weight_grads(a4, dz)
        check("dWh", dwh, rw, R.gamma(B + 1) * tw)
        check("dbh", dbh, rb, R.gamma(B + 1) * tb)
        d4, t4 = R.backward_data(a4, wh, dz, w4, dq if with_dq else None)
        coeff = R.gamma(width + 3) + (R.gamma(B) if B > 1 else 0.0)
        check("db3 (dz4)", g[7], d4.sum(axis=0), coeff * t4.sum(axis=0))
        if with_dq:
            r4, rb4, t4w, t4b = R.weight_grads(a4, dq)
            check("dW4", g[8], r4, R.gamma(B + 1) * t4w)
            check("db4", g[9], rb4, R.gamma(B + 1) * t4b)
        else:
            assert not g[8].any() and not g[9].any()
    T.close()


def test_identity_head_returns_a4(world):
    """a width-512 identity head: Z is a4 exactly (every other product of a chain is a zero)"""
    B = 5
    T = net()
    head = T.attach_head(512)
    head.set(0, np.eye(512, dtype=np.float32))
    src = source(world, B, 7)
    _, z, _ = forward_both(T, src)
    assert same(z, a4_of(T.model, B))
    T.close()


# ---------------------------------------------------------------- 4. clip_by_norm and Adam

@pytest.mark.parametrize("clipped", [True, False])
@pytest.mark.parametrize("width", WIDTHS)
def test_clip_and_adam_against_the_restatement(world, width, clipped):
    """The head's first update against clip_adam of the restatement fed the GPU's own raw gradients, per variable v of n_v
    elements (Wh: 512 width, bh: width).  Tolerance of a weight: 2 ulp of it + lr rho / 4, rho = gamma(n_v + 2).
    Derivation: the clipped gradient g = raw * clipnorm / max(norm, clipnorm) carries the relative error of the norm - a sum
    of n_v squares, gamma(n_v + 1) / 2 after the root - and three roundings of its own: at most rho.  From m = v = 0 the
    update moves a weight by lr g / (|g| + e'), e' = eps / sqrt(1 - beta2), whose derivative in g is e' / (|g| + e')^2; a
    relative error rho in g therefore moves it by lr rho |g| e' / (|g| + e')^2 <= lr rho / 4 (the maximum is at |g| = e').
    The float32 evaluation of the step itself and the final subtraction stay within 2 ulp of the weight.  m = (1 - beta1) g
    and v = (1 - beta2) g^2 carry g's error once and twice, plus their own roundings.
    clipped: dz is scaled so that the smaller of the two norms is 2 clipnorm; otherwise so that the larger is clipnorm / 2
    (the scale comes from the restatement's gradient of the unscaled dz)."""
    B = 5
    T = net()
    head = T.attach_head(width, seed=3)
    rng = np.random.default_rng(width)
    head.set(1, rng.normal(size=width).astype(np.float32))
    src = source(world, B, width)
    _, _, ticket = forward_both(T, src)
    hp = qlx.model_hparams()
    lr, clip = float(hp[0]), float(hp[4])
    dz = rng.normal(size=(B, width))
    rw, rb, _, _ = R.weight_grads(a4_of(T.model, B), dz.astype(np.float32))
    norms = [float(np.sqrt((rw * rw).sum())), float(np.sqrt((rb * rb).sum()))]
    scale = 2 * clip / min(norms) if clipped else clip / (2 * max(norms))
    dz = (scale * dz).astype(np.float32)
    T.backward_dz(dev(dz), None, ticket, **src)
    graw = head_grads_host(T)
    before = [[head.get(var, which) for which in range(3)] for var in range(2)]
    model_before = [T.model.get(v) for v in range(qlx.NUM_VARS)]
    T.step()
    T.sync()
    assert head.iterations() == 1
    print(f"width {width}, clipped {clipped}, scale {scale:.3g}")
    for var, n_v in ((0, 512 * width), (1, width)):
        w0, m0, v0 = before[var]
        assert not m0.any() and not v0.any()
        w, m, v, norm = R.clip_adam(w0, m0, v0, graw[var], 1, hp)
        assert (norm > clip) == clipped, (var, norm)
        rho = R.gamma(n_v + 2)
        gw, gm, gv = (head.get(var, which) for which in range(3))
        ulp = np.spacing(np.maximum(np.abs(w0), np.abs(w).astype(np.float32)))
        check(f"var {var} w (norm {norm:.3g})", gw, w, 2 * ulp.astype(np.float64) + lr * rho / 4)
        check(f"var {var} m", gm, m, (rho + 4 * R.U) * np.abs(m) + 1e-45)
        check(f"var {var} v", gv, v, (2 * rho + 8 * R.U) * np.abs(v) + 1e-45)
        assert np.abs(gw - w0).max() > 0
    # the model stepped with it, on its own gradient
    assert not same(T.model.get(6), model_before[6])
    T.close()


def test_other_backwards_leave_the_head_alone(world):
    B = 5
    T = net()
    head = T.attach_head(17)
    src = source(world, B, 1)
    _, _, ticket = forward_both(T, src)
    T.backward_dz(dev(np.ones((B, 17), np.float32)), None, ticket, **src)
    T.discard_grad()
    w0 = head.get(0)
    T.backward_dq(dev(np.ones((B, 3), np.float32)), 0, **src)   # the model's own backward after the head's
    T.step()
    T.train(dev(np.zeros(B, np.uint8)), dev(np.ones(B, np.float32)), **src)
    T.sync()
    assert T.model.iterations() == 2 and head.iterations() == 0
    assert same(head.get(0), w0)
    T.close()


# ---------------------------------------------------------------- 6. state errors

def test_state_errors(world):
    L = qlx.lib()
    T = net(reserve=8)
    head = T.attach_head(4)
    with pytest.raises(qlx.QlError, match="status -4"):
        qlx.WideHead(T.model, 4)
    # the model cannot go while its head lives
    assert L.qlx_model_destroy(T.h) == -4
    assert b"head" in L.qlx_last_error()
    # n above the reserve: QLX_E_STATE, nothing launched (the forward ticket stands)
    obs = torch.zeros((16, 4, 84, 84), dtype=torch.uint8, device=DEV)
    z = torch.zeros((16, 4), dtype=torch.float32, device=DEV)
    s = qlx.StatesDev(obs=obs.data_ptr(), layout=qlx.OBS_NCHW_TIME)
    ticket = T.forward_ticket()
    assert L.qlx_head_forward_dev(head.h, C.byref(s), 16, z.data_ptr(), None) == -4
    assert b"reserve" in L.qlx_last_error()
    assert L.qlx_head_backward_dev(head.h, C.byref(s), z.data_ptr(), None, 16, 0) == -4
    assert T.forward_ticket() == ticket
    T.sync()
    assert not host(z).any()
    # a replay index >= len: the zero state and the sticky flag, as qlx_model_q_dev
    _, rb = world
    with torch.no_grad():
        _, zbad = T.forward(head=True, replay=rb, indices=dev(np.array([len(rb) + 3], np.int64)), layout=LAY)
        _, zzero = T.forward(obs[:1], head=True, layout=LAY)
    assert same(host(zbad), host(zzero))
    with pytest.raises(qlx.QlError, match="index"):
        T.sync()
    # after the head is gone the model can take another one, and can go
    head.close()
    again = T.attach_head(5)
    assert again.width == 5
    T.close()
    assert T.h is None and again.h is None


def test_bf16_model_takes_no_head():
    T = net(arch="bf16", reserve=8)
    with pytest.raises(qlx.QlError, match="status -1"):
        T.attach_head(4)
    T.close()
