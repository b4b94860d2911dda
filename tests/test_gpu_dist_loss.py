"""The distributional losses on the wide head on the GPU (include/qlx.h "distributional losses on the wide head", DESIGN.md
§20; csrc/dist_loss.hip), driven through qlx_torch.TorchQNet.head_values / dist_loss / train_dist and the C calls.

1. Quantile loss and values: the same bits as the float32 restatement (tests/dist_loss_reference.py (a)).
2. The N = 1 pin: a width-3 head holding W4 and b4 gives 0.5 x the built-in Huber head's dq and trunk gradients, bit for bit.
3. Categorical loss and values against the float64 restatement (b), within the bound that restatement derives.
4. Determinism and independence of the batch, both kinds.
5. train_dist is the four calls, bit for bit.
6. State errors.
All comparisons are made on bytes copied back to the host; "the same bits" compares the 32-bit patterns.

Largest categorical error / bound measured on an MI355X (test 3; expf and logf counted as 2 ulp each): see DESIGN.md §20."""
import ctypes as C

import numpy as np
import pytest
import torch

import qlx_torch as QT   # before any other use of qlx in this process (it checks that itself)
import qlx

import dist_loss_reference as R

pytestmark = pytest.mark.gpu

SEED = 0x51A5EED
DEV = "cuda:0"
LAY = "nchw_time"
N_ENVS, CAP, STEPS = 4, 128, 30
BATCHES = [1, 5, 100]
Q_ATOMS = [1, 2, 51, 64, 65, 200, 341]   # one quantile; one wave, ragged; one full wave; a second wave; one thread row, ragged;
C_ATOMS = [2, 3, 51, 64, 65, 341]        # 341: the second thread row (N > 256) and the largest head


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
    _, rb = world
    rng = np.random.default_rng(1000 + seed)
    rest = rng.permutation(np.delete(np.arange(len(rb)), 77))[:B - 1]
    idx = np.concatenate([[77], rest]).astype(np.int64)
    return dict(replay=rb, indices=dev(idx), layout=LAY)


def make_batch(rng, B, N, scale=1.5):
    """host arrays of one batch: Z and z_next seeded normals (scale 1.5: |u| on both sides of 1, both signs)"""
    return dict(z=(scale * rng.normal(size=(B, 3 * N))).astype(np.float32),
                actions=rng.integers(0, 3, B).astype(np.uint8),
                returns=rng.normal(size=B).astype(np.float32),
                discounts=np.full(B, 0.99 ** 3, np.float32),
                terminals=(rng.random(B) < 0.2).astype(np.uint8),
                z_next=(scale * rng.normal(size=(B, 3 * N))).astype(np.float32))


def run_loss(T, dist, b, a_star=None, weights=None):
    """TorchQNet.dist_loss on host arrays -> host dict"""
    with torch.no_grad():
        loss, dz, sl, a = T.dist_loss(dev(b["z"]), dist, dev(b["actions"]), dev(b["returns"]), dev(b["discounts"]),
                                      dev(b["terminals"]), dev(b["z_next"]), None if a_star is None else dev(a_star),
                                      None if weights is None else dev(weights))
    T.sync()
    return dict(loss=host(loss), dz=host(dz), sample_loss=host(sl), a_star=host(a))


# ---------------------------------------------------------------- 1. quantile: bit for bit

def directed_quantile_rows(b, B, N):
    """row 0: a terminal sample whose target is the return 0.5, with theta 0.5 (u == 0), -0.5 (u == 1) and 1.5 (u == -1) as
    far as N has room; row 1 (B > 1): action 2, and action 0 of z_next raised so that a* is 0, not terminal"""
    z = b["z"].reshape(B, 3, -1)
    b["terminals"][0], b["returns"][0], b["actions"][0] = 1, 0.5, 1
    for i, v in enumerate([0.5, -0.5, 1.5][:N]):
        z[0, 1, i] = v
    if B > 1:
        b["terminals"][1], b["actions"][1] = 0, 2
        b["z_next"].reshape(B, 3, -1)[1, 0] += np.float32(5)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("N", Q_ATOMS)
def test_quantile_loss_is_the_float32_restatement(N, B):
    T = net()
    T.attach_head(3 * N)
    dist = QT.Quantile(N)
    rng = np.random.default_rng(7 * N + B)
    b = make_batch(rng, B, N)
    directed_quantile_rows(b, B, N)
    w = (rng.random(B) + 0.5).astype(np.float32)
    other = rng.integers(0, 3, B).astype(np.uint8)
    if B > 1:
        other[1] = 0
    for a_star in (None, other):
        for weights in (None, w):
            got = run_loss(T, dist, b, a_star, weights)
            ref = R.quantile32(N=N, a_star=a_star, weights=weights, **b)
            assert np.array_equal(got["a_star"], ref["a_star"])
            if B > 1:
                assert got["a_star"][1] == 0 and b["actions"][1] == 2
            assert same(got["sample_loss"], ref["sample_loss"]), float(np.abs(got["sample_loss"] - ref["sample_loss"]).max())
            assert same(got["dz"], ref["dz"]), float(np.abs(got["dz"] - ref["dz"]).max())
            assert same(got["loss"], ref["loss"]), (float(got["loss"]), float(ref["loss"]))
            assert np.isfinite(got["dz"]).all() and (np.abs(got["dz"]).max() > 0 or N * B == 1)   # (alone, u == 0 is all there is)
    # the directed terms are there: u == 0 contributes nothing, |u| == 1 sits on the quadratic side of the branch
    zr = b["z"].reshape(B, 3, N)[0, 1]
    assert zr[0] == b["returns"][0] and (N < 2 or b["returns"][0] - zr[1] == 1) and (N < 3 or b["returns"][0] - zr[2] == -1)
    T.close()


@pytest.mark.parametrize("N", Q_ATOMS)
def test_quantile_values_are_the_float32_restatement(N):
    n = 37   # ten blocks of four waves, the last one ragged
    T = net()
    T.attach_head(3 * N)
    rng = np.random.default_rng(N)
    z = (1.5 * rng.normal(size=(n, 3, N))).astype(np.float32)
    z[3, 2] = z[3, 1]          # an exact tie of the two best: the first of them
    z[3, 0] = z[3, 1] - np.float32(1)
    z[4, 1] = z[4, 0]          # all three equal: action 0
    z[4, 2] = z[4, 0]
    q, a, mq = (host(t) for t in T.head_values(dev(z.reshape(n, 3 * N)), QT.Quantile(N)))
    T.sync()
    rq, ra, rmq = R.values32_quantile(z, N)
    assert same(q, rq) and np.array_equal(a, ra) and same(mq, rmq)
    assert a[3] == 1 and a[4] == 0 and q[3, 1] == q[3, 2] and len(set(a.tolist())) == 3
    only = host(T.head_values(dev(z.reshape(n, 3 * N)), QT.Quantile(N), want="max_q"))
    assert same(only, rmq)
    T.close()


# ---------------------------------------------------------------- 2. the N = 1 pin

def test_one_quantile_is_half_the_huber_head(world):
    """A width-3 head holding W4 and b4 read as one quantile per action, z_next the target's Q, no weights: tau = 0.5, so
    omega = 0.5 either way, the loss is half the Huber loss and dz exactly 0.5 x the built-in head's
    dq = (1 * clamp(q_a - y, -1, 1)) / B with y = returns + live * max Q' (csrc/qnet32.hip, the training head)."""
    B = 33
    A, T, G = net(), net(), net(seed=11)
    head = T.attach_head(3, seed=9)
    head.set(0, A.model.get(8))
    head.set(1, A.model.get(9))
    src = source(world, B, 3)
    rng = np.random.default_rng(5)
    qA = host(A.q(want="q", **src))
    tA = A.forward_ticket()
    q_next = host(G.q(want="q", replay=src["replay"], indices=src["indices"], which="s_next", layout=LAY))
    actions = rng.integers(0, 3, B).astype(np.uint8)
    returns = rng.normal(size=B).astype(np.float32)
    discounts = np.full(B, 0.97, np.float32)
    terminals = (rng.random(B) < 0.2).astype(np.uint8)
    returns[:2] = qA[np.arange(2), actions[:2]] + np.float32([3, -3])   # both linear sides of the Huber branch
    terminals[:2] = 1
    live = np.where(terminals != 0, np.float32(0), discounts).astype(np.float32)
    y = returns + live * q_next.max(axis=1)
    e = qA[np.arange(B), actions] - y
    dq = np.zeros((B, 3), np.float32)
    dq[np.arange(B), actions] = (np.float32(1) * np.clip(e, np.float32(-1), np.float32(1))) / np.float32(B)
    assert (np.abs(e) > 1).any() and (np.abs(e) < 1).any()
    dist = QT.Quantile(1)
    args = (dev(actions), dev(returns), dev(discounts), dev(terminals), dev(q_next))
    with torch.no_grad():
        _, z = T.forward(head=True, **src)
        loss, dz, sl, a_star = T.dist_loss(z, dist, *args)
    assert same(host(z), qA)
    dz = host(dz)
    assert np.array_equal(host(a_star), q_next.argmax(axis=1))
    normal = (np.abs(dq) >= 2.0 ** -125)
    assert normal.sum() >= B - 2
    assert np.array_equal(bits(dz)[normal], bits(np.float32(0.5) * dq)[normal]) and not dz[dq == 0].any()
    # the whole update: the trunk's raw gradients are half of the model's own backward for that dq
    A.backward_dq(dev(dq), tA, **src)
    gA = [host(g) for g in A.grads()]
    loss2, _ = T.train_dist(dist, *args, **src)
    gT = [host(g) for g in T.grads()]
    T.sync(), A.sync()
    assert same(host(loss2), host(loss))
    for v in range(8):
        big = np.abs(gA[v]) >= 2.0 ** -120
        assert big.any(), v
        assert np.array_equal(bits(gT[v])[big], bits(np.float32(0.5) * gA[v])[big]), v
    assert head.iterations() == 1 and T.model.iterations() == 1
    A.close(), T.close(), G.close()


# ---------------------------------------------------------------- 3. categorical against float64

WORST = {}


def check(name, got, ref, bound):
    err = np.abs(np.asarray(got, np.float64) - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    WORST[name] = max(WORST.get(name, 0.0), worst)
    print(f"  {name}: max err / bound = {worst:.3g} (max so far {WORST[name]:.3g}), max |ref| = {float(np.abs(ref).max()):.3g}")
    assert np.isfinite(got).all(), name
    assert (err <= bound).all(), (name, worst)
    return worst


def categorical_batch(rng, B, N, v_min, v_max):
    b = make_batch(rng, B, N, scale=1.0)
    span = v_max - v_min
    b["returns"] = (v_min + span * (1.4 * rng.random(B) - 0.2)).astype(np.float32)   # some clipped at either end
    b["terminals"][0] = 1
    b["returns"][0] = np.float32(v_min + span * (N // 2) / (N - 1))                  # on (or next to) an atom
    return b


@pytest.mark.parametrize("v_min,v_max", [(-10.0, 10.0), (0.0, 1.0)])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("N", C_ATOMS)
def test_categorical_loss_against_the_float64_restatement(N, B, v_min, v_max):
    """L_b, the loss, dz and Q within the bound categorical64(bounds=True) propagates through the kernel's operations from
    u = 2^-24 per fp32 operation and 2 ulp for expf and logf (counted, the ROCm accuracy tables are not in the tree).  The
    restatement is fed the GPU's a*; separately the GPU's a* must be the float64 argmax wherever the float64 top-two gap
    exceeds the bounds of the two values."""
    T = net()
    T.attach_head(3 * N)
    dist = QT.Categorical(N, v_min, v_max)
    rng = np.random.default_rng(13 * N + B)
    b = categorical_batch(rng, B, N, v_min, v_max)
    w = (rng.random(B) + 0.5).astype(np.float32)
    print(f"N {N}, B {B}, [{v_min}, {v_max}]")
    for weights in (None, w):
        got = run_loss(T, dist, b, None, weights)
        ref = R.categorical64(N=N, v_min=v_min, v_max=v_max, a_star=got["a_star"], weights=weights, bounds=True, **b)
        check("L_b", got["sample_loss"], ref["sample_loss"], ref["err_sample_loss"])
        check("loss", got["loss"], ref["loss"], ref["err_loss"])
        check("dz", got["dz"], ref["dz"], ref["err_dz"])
        assert np.abs(ref["dz"]).max() > 0 and abs(ref["m"].sum(axis=1) - 1).max() < 1e-9
        other = ((got["a_star"] + 1) % 3).astype(np.uint8)
        got2 = run_loss(T, dist, b, other, weights)
        ref2 = R.categorical64(N=N, v_min=v_min, v_max=v_max, a_star=other, weights=weights, bounds=True, **b)
        assert np.array_equal(got2["a_star"], other)
        check("dz (a* given)", got2["dz"], ref2["dz"], ref2["err_dz"])
        check("L_b (a* given)", got2["sample_loss"], ref2["sample_loss"], ref2["err_sample_loss"])
    # values, and a*
    q, a, mq = (host(t) for t in T.head_values(dev(b["z_next"]), dist))
    T.sync()
    rq, ra, rmq, eq = R.values64_categorical(b["z_next"], N, v_min, v_max, bounds=True)
    check("Q", q, rq, eq)
    assert np.array_equal(a, got["a_star"]), "the loss kernel and the values kernel choose differently"
    assert same(mq, q[np.arange(B), a])
    top2 = np.sort(rq, axis=1)[:, 1:]
    clear = (top2[:, 1] - top2[:, 0]) > 2 * eq.max(axis=1)
    assert np.array_equal(a[clear], ra[clear])
    T.close()


def test_categorical_inputs_have_clear_argmaxes():
    """a condition on the test's inputs, checked without the GPU's results: at least 95 % of all samples of test 3 have a
    float64 top-two gap above the bound"""
    clear = total = 0
    for v_min, v_max in [(-10.0, 10.0), (0.0, 1.0)]:
        for N in C_ATOMS:
            for B in BATCHES:
                b = categorical_batch(np.random.default_rng(13 * N + B), B, N, v_min, v_max)
                rq, _, _, eq = R.values64_categorical(b["z_next"], N, v_min, v_max, bounds=True)
                top2 = np.sort(rq, axis=1)[:, 1:]
                clear += int(((top2[:, 1] - top2[:, 0]) > 2 * eq.max(axis=1)).sum())
                total += B
    print(f"clear argmaxes: {clear} of {total}")
    assert clear >= 0.95 * total


def test_categorical_extreme_logits_stay_finite():
    N, B = 51, 5
    T = net()
    T.attach_head(3 * N)
    dist = QT.Categorical(N, -10.0, 10.0)
    rng = np.random.default_rng(1)
    b = categorical_batch(rng, B, N, -10.0, 10.0)
    b["z"] = np.where(rng.random((B, 3 * N)) < 0.5, np.float32(60), np.float32(-60)).astype(np.float32)
    b["z_next"] = np.where(rng.random((B, 3 * N)) < 0.5, np.float32(60), np.float32(-60)).astype(np.float32)
    got = run_loss(T, dist, b)
    ref = R.categorical64(N=N, v_min=-10.0, v_max=10.0, a_star=got["a_star"], bounds=True, **b)
    for k in ("loss", "dz", "sample_loss"):
        assert np.isfinite(got[k]).all(), k
    check("L_b (+-60)", got["sample_loss"], ref["sample_loss"], ref["err_sample_loss"])
    check("dz (+-60)", got["dz"], ref["dz"], ref["err_dz"])
    q = host(T.head_values(dev(b["z"]), dist, want="q"))
    assert np.isfinite(q).all() and (q >= -10).all() and (q <= 10).all()
    T.close()


# ---------------------------------------------------------------- 4. determinism and independence

@pytest.mark.parametrize("kind", ["quantile", "categorical"])
def test_a_sample_does_not_see_its_batch(kind):
    """Sample 0 alone (B = 1, weight 1) and first in a batch of 100 with every weight 100: L_b and a* are the same bits;
    dz = (w g) / B differs by the two roundings of (100 g) / 100, 2 u |dz|.  Two runs give the same bits everywhere."""
    N, B = 65, 100
    T = net()
    T.attach_head(3 * N)
    dist = QT.Quantile(N) if kind == "quantile" else QT.Categorical(N, -10.0, 10.0)
    rng = np.random.default_rng(9)
    b = make_batch(rng, B, N) if kind == "quantile" else categorical_batch(rng, B, N, -10.0, 10.0)
    w = np.full(B, 100, np.float32)
    got = run_loss(T, dist, b, None, w)
    again = run_loss(T, dist, b, None, w)
    for k in got:
        assert same(got[k], again[k]), k
    one = run_loss(T, dist, {k: v[:1] for k, v in b.items()})
    assert same(one["sample_loss"], got["sample_loss"][:1]) and np.array_equal(one["a_star"], got["a_star"][:1])
    assert np.abs(one["dz"]).max() > 0
    assert (np.abs(R.f64(one["dz"][0]) - R.f64(got["dz"][0])) <= 2 * R.U * np.abs(R.f64(one["dz"][0])) + 2.0 ** -149).all()
    # and last in the batch: the position does not matter
    flip = {k: v[::-1].copy() for k, v in b.items()}
    back = run_loss(T, dist, flip, None, w)
    assert same(back["sample_loss"][::-1], got["sample_loss"]) and same(back["dz"][::-1], got["dz"])
    T.close()


# ---------------------------------------------------------------- 5. train_dist is the four calls

def by_parts(T, dist, args, src, loss, sl):
    """qlx_head_forward_dev (no q), qlx_head_dist_loss_dev, qlx_head_backward_dev with that ticket, qlx_model_step_dev(0)"""
    L, head = qlx.lib(), T.head
    s, B, ins = T._source(None, None, src["replay"], src["indices"], "s", LAY)
    batch, ts = T._dist_batch(B, dist, *args)
    z = torch.empty((B, dist.width), dtype=torch.float32, device=DEV)
    dz = torch.empty((B, dist.width), dtype=torch.float32, device=DEV)
    T._run(None, src["replay"], ins + (z,), lambda: L.qlx_head_forward_dev(head.h, C.byref(s), B, z.data_ptr(), None))
    ticket = T.forward_ticket()
    T._run(None, None, ts + (z, dz, loss, sl),
           lambda: L.qlx_head_dist_loss_dev(head.h, C.byref(dist.c), z.data_ptr(), C.byref(batch), B, dz.data_ptr(),
                                            loss.data_ptr(), sl.data_ptr(), None))
    T._run(None, src["replay"], ins + (dz,), lambda: L.qlx_head_backward_dev(head.h, C.byref(s), dz.data_ptr(), None, B, ticket))
    T._run(None, None, (), lambda: L.qlx_model_step_dev(T.h, 0))


@pytest.mark.parametrize("kind", ["quantile", "categorical"])
def test_train_dist_is_the_four_calls(world, kind):
    N, B = 51, 37
    dist = QT.Quantile(N) if kind == "quantile" else QT.Categorical(N, -10.0, 10.0)
    nets = [net(seed=5), net(seed=5)]
    for T in nets:
        T.attach_head(3 * N, seed=8)
    rng = np.random.default_rng(3)
    losses = [[], []]
    for upd in range(2):
        b = make_batch(rng, B, N) if kind == "quantile" else categorical_batch(rng, B, N, -10.0, 10.0)
        w = (rng.random(B) + 0.5).astype(np.float32)
        src = source(world, B, upd)
        args = (dev(b["actions"]), dev(b["returns"]), dev(b["discounts"]), dev(b["terminals"]), dev(b["z_next"]), None, dev(w))
        loss, sl = nets[0].train_dist(dist, *args, want_sample_loss=True, **src)
        loss2 = torch.empty((), dtype=torch.float32, device=DEV)
        sl2 = torch.empty(B, dtype=torch.float32, device=DEV)
        by_parts(nets[1], dist, args, src, loss2, sl2)
        losses[0].append((host(loss), host(sl)))
        losses[1].append((host(loss2), host(sl2)))
    for T in nets:
        T.sync()   # clean: no flag
    for (l0, s0), (l1, s1) in zip(*losses):
        assert same(l0, l1) and same(s0, s1) and np.isfinite(l0) and l0 > 0
    A, P = nets
    assert A.model.iterations() == P.model.iterations() == 2 and A.head.iterations() == P.head.iterations() == 2
    moved = 0
    for which in range(3):
        for v in range(qlx.NUM_VARS):
            assert same(A.model.get(v, which), P.model.get(v, which)), (v, which)
        for var in range(2):
            assert same(A.head.get(var, which), P.head.get(var, which)), (var, which)
            moved += int(np.abs(A.head.get(var, which)).max() > 0)
    assert moved == 6
    fresh = net(seed=5)
    assert not same(A.model.get(0), fresh.model.get(0)), "the trunk did not move"
    # an action of 3 trains as action 0 and is reported once
    b["actions"][4] = 3
    A.train_dist(dist, dev(b["actions"]), *args[1:], **src)
    with pytest.raises(qlx.QlError, match="action"):
        A.sync()
    A.sync()
    for T in nets + [fresh]:
        T.close()


# ---------------------------------------------------------------- 6. state errors

def test_state_errors(world):
    L = qlx.lib()
    T = net(reserve=8)
    head = T.attach_head(153)
    z = torch.zeros((16, 153), dtype=torch.float32, device=DEV)
    dz = torch.full((16, 153), 7.0, dtype=torch.float32, device=DEV)
    q = torch.full((16, 3), 7.0, dtype=torch.float32, device=DEV)
    u8 = torch.zeros(16, dtype=torch.uint8, device=DEV)
    f = torch.zeros(16, dtype=torch.float32, device=DEV)
    batch = qlx.DistBatch(u8.data_ptr(), f.data_ptr(), f.data_ptr(), u8.data_ptr(), z.data_ptr(), None, None)
    obs = torch.zeros((16, 4, 84, 84), dtype=torch.uint8, device=DEV)
    s = qlx.StatesDev(obs=obs.data_ptr(), layout=qlx.OBS_NCHW_TIME)
    good, wrong = qlx.Dist(qlx.DIST_QUANTILE, 51, 0, 0), qlx.Dist(qlx.DIST_QUANTILE, 50, 0, 0)
    calls = lambda d, n: (   # noqa: E731
        L.qlx_head_values_dev(head.h, C.byref(d), z.data_ptr(), n, q.data_ptr(), None, None),
        L.qlx_head_dist_loss_dev(head.h, C.byref(d), z.data_ptr(), C.byref(batch), n, dz.data_ptr(), None, None, None),
        L.qlx_head_dist_train_dev(head.h, C.byref(d), C.byref(s), C.byref(batch), n, z.data_ptr(), dz.data_ptr(), None, None))
    ticket = T.forward_ticket()
    # a descriptor that does not fit the width
    for status in calls(wrong, 4):
        assert status == -1 and b"atoms" in L.qlx_last_error()
    # n above the reserve
    for status in calls(good, 16):
        assert status == -4 and b"reserve" in L.qlx_last_error()
    assert T.forward_ticket() == ticket and T.model.iterations() == 0 and head.iterations() == 0
    T.sync()
    assert (host(dz) == 7).all() and (host(q) == 7).all(), "a failed call launched something"
    with pytest.raises(ValueError, match="width"):
        T.head_values(z[:4], QT.Quantile(50))
    T.close()
    # a bf16 model has no head to take a distributional loss
    H = net(arch="bf16", reserve=8)
    with pytest.raises(qlx.QlError, match="status -1"):
        H.attach_head(153)
    with pytest.raises(RuntimeError, match="attach_head"):
        H.head_values(z[:4], QT.Quantile(51))
    H.close()
