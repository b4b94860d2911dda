"""The Q-net's device-tensor calls through qlx_torch.TorchQNet on the GPU (include/qlx.h "Q-network on device tensors",
DESIGN.md §16), bit for bit against the host calls they stand beside (qlx_model_predict, qlx_model_batch_max_q,
qlx_model_train) and against the learner's own update.  Nothing here has a tolerance: both paths run the same kernels on the
same frame tables, so every result is compared as bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

import qlx_torch as QT   # before any other use of qlx in this process (it checks that itself)
import qlx

pytestmark = pytest.mark.gpu

SEED = 0x51A5EED
DEV = "cuda:0"
ARCHS = ["f32", "bf16"]
LAYOUTS = ["nhwc_slot", "nchw_time"]
PREC = {"f32": qlx.PREC_F32, "bf16": qlx.PREC_BF16}
PER_SAMPLE = (12800, 5184, 3136, 512)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def host(t):
    return None if t is None else t.cpu().numpy()


def dev(a, dtype=None):
    return torch.as_tensor(np.array(a, order="C"), dtype=dtype).to(DEV)   # (a copy: the shared references are read-only)


def net(arch, seed=2, reserve=64, env=None):
    return QT.TorchQNet(arch, seed=seed, device=DEV, env=env, reserve=reserve)


def activation(m, layer, n):
    got = np.zeros(n * PER_SAMPLE[layer - 1], np.float32)
    assert qlx.lib().qlx_model_last_activation(m.h, layer, got.ctypes.data_as(C.c_void_p)) == 0
    return got


def model_state(model):
    """weights, Adam m and v of all ten variables, and the iteration count"""
    return [model.get(v, w) for v in range(qlx.NUM_VARS) for w in range(3)], model.iterations()


def same_state(a, b):
    return a[1] == b[1] and all(same(x, y) for x, y in zip(a[0], b[0]))


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


# ---------------------------------------------------------------- 1. dense states against the host calls

@pytest.fixture(scope="module")
def pool():
    """257 states: uniformly random bytes (every one of the 28,224 positions matters to conv1), eight real env states three
    steps into an episode (ring slot 3 is still a zero frame) and one all-zero state, the three kinds within the first 3"""
    rng = np.random.default_rng(11)
    x = rng.integers(0, 256, (257, 84, 84, 4), dtype=np.uint8)
    env = qlx.BreakoutEnvironment(8, SEED)
    for _ in range(3):
        env.step(rng.integers(0, 3, 8).astype(np.uint8))
    st = env.state()
    env.close()
    assert st[..., :3].any() and not st[..., 3].any()
    x[1] = st[0]
    x[2] = 0
    x[3:10] = st[1:]
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module")
def fwd_nets():
    """one model per arch for the tests that never train it"""
    nets = {a: net(a, reserve=264) for a in ARCHS}
    yield nets
    for m in nets.values():
        m.close()


@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("n", [1, 3, 33, 257])
def test_dense_source_equals_host_calls(fwd_nets, pool, arch, n):
    m = fwd_nets[arch]
    x = pool[:n]
    q_ref, a_ref = m.model.q_values(x)
    a1_ref = activation(m, 1, n)
    mq_ref = m.model.batch_predict_max_future_reward(x)
    xd = dev(x)
    other = dev(255 - x)
    for layout, states, clobber in (("nhwc_slot", xd, other), ("nchw_time", nchw(xd), nchw(other))):
        # the host calls staged these very frames in the model's workspace: overwrite them first, so that what follows is
        # the pack kernel's own work
        q0 = m.q(clobber, layout=layout, want="q")
        assert not same(host(q0), q_ref)
        q, a, mq = m.q(states, layout=layout)
        m.sync()
        assert same(activation(m, 1, n), a1_ref), f"{layout}: conv1's output pins every packed byte"
        assert same(host(q), q_ref) and same(host(a), a_ref) and same(host(mq), mq_ref), layout
        only_a = m.q(states, layout=layout, want="actions")
        only_mq = m.q(states, layout=layout, want=("max_q",))[0]
        assert same(host(only_a), a_ref) and same(host(only_mq), mq_ref)
    out = {"q": torch.full((n, 3), 7.0, device=DEV)}
    got = m.q(xd, layout="nhwc_slot", want=("q",), out=out)[0]
    assert got is out["q"] and same(host(got), q_ref)
    m.sync()


# ---------------------------------------------------------------- 2. env source

@pytest.mark.parametrize("arch", ARCHS)
def test_env_source(arch):
    n = 33
    te = QT.TorchEnv(n, SEED, DEV)
    rng = np.random.default_rng(5)
    for t in range(6):
        te.step(dev(rng.integers(0, 3, n).astype(np.uint8)))
        if t == 2:   # these envs start again: their older channels are zero frames, next_slot differs between envs
            te.reset(dev((np.arange(n) % 4 == 1).astype(np.uint8)))
    assert len(set(te.mechanics()["next_slot"].tolist())) > 1
    shared, own = net(arch, env=te, reserve=n), net(arch, reserve=n)
    assert shared.stream.cuda_stream == te.stream.cuda_stream != own.stream.cuda_stream
    for layout in LAYOUTS:
        ref = [host(t) for t in own.q(te.obs(layout), layout=layout)]
        for m in (shared, own):
            got = [host(t) for t in m.q(env=te, layout=layout)]
            assert all(same(g, r) for g, r in zip(got, ref)), layout
        if layout == "nhwc_slot":
            q_host, a_host = own.model.q_values(te._env.state())
            assert same(ref[0], q_host) and same(ref[1], a_host)
    with pytest.raises(ValueError):
        net(arch, reserve=n - 1).q(env=te)
    te.sync(), shared.sync(), own.sync()
    own.close()
    te.close()   # closes the model that shares its stream first
    assert shared.h is None


# ---------------------------------------------------------------- 3. replay source

N_ENVS, CAP, T = 3, 37, 20


class World:
    """3 envs, capacity 37, 20 vector steps = 60 pushes through device tensors: the ring wraps and 37 is no multiple of 3.
    Env 0 is given a done at step 10 and reset, env 1 is reset without a done after step 13, env 2 plays on, so the live
    transitions have episode steps 1, 2, 3, ... (zero frames, every ring phase) and 8 .. 20."""

    def __init__(self):
        self.env = QT.TorchEnv(N_ENVS, SEED, DEV)
        self.rb = QT.TorchReplay(CAP, self.env)
        rng = np.random.default_rng(17)
        for t in range(T):
            a = dev(rng.integers(0, 3, N_ENVS).astype(np.uint8))
            _, d = self.env.step(a)
            rewards = dev(rng.standard_normal(N_ENVS).astype(np.float32))
            cut = np.zeros(N_ENVS, np.uint8)
            if t == 9:
                d = d | dev(np.array([1, 0, 0], np.uint8))
                cut[0] = 1
            if t == 12:
                cut[1] = 1
            self.rb.add(self.env, a, rewards, d)
            if cut.any():
                self.env.reset(dev(cut))
        self.rb.sync()
        assert len(self.rb) == CAP
        self.all = dev(np.arange(CAP, dtype=np.int64))

    def indices(self, B):
        return dev(((np.arange(B, dtype=np.int64) * 7 + 3) % CAP))


@pytest.fixture(scope="module")
def world():
    return World()


@pytest.mark.parametrize("arch", ARCHS)
def test_replay_source(fwd_nets, world, arch):
    m, rb = fwd_nets[arch], world.rb
    for layout in LAYOUTS:
        b = rb.batch(world.all, layout=layout)
        for which, states in (("s", b.s), ("s_next", b.s_next)):
            ref = [host(t) for t in m.q(states, layout=layout)]
            got = [host(t) for t in m.q(replay=rb, indices=world.all, which=which, layout=layout)]
            assert all(same(g, r) for g, r in zip(got, ref)), (layout, which)
        b3 = rb.batch(world.all, n_step=3, layout=layout)
        assert not same(host(b3.last_indices), host(world.all))
        ref = host(m.q(b3.s_next, layout=layout, want="q"))
        got = host(m.q(replay=rb, indices=b3.last_indices, which="s_next", layout=layout, want="q"))
        assert same(got, ref), layout
    m.sync()
    rb.sync()


@pytest.mark.parametrize("arch", ARCHS)
def test_replay_index_out_of_range(fwd_nets, world, arch):
    m, rb = fwd_nets[arch], world.rb
    good = host(m.q(replay=rb, indices=world.all, want="q"))
    zero = host(m.q(torch.zeros((1, 4, 84, 84), dtype=torch.uint8, device=DEV), want="q"))
    m.sync()
    idx = world.all.clone()
    idx[5] = CAP   # == len
    idx[20] = -1   # the ABI's uint64: far above len
    got = host(m.q(replay=rb, indices=idx, want="q"))
    with pytest.raises(qlx.QlError, match="index"):
        m.sync()
    m.sync()   # reported once
    expect = good.copy()
    expect[5] = expect[20] = zero[0]
    assert same(got, expect) and not same(good[5], zero[0])
    rb.sync()   # the flag is the model's, not the replay's


# ---------------------------------------------------------------- 4. / 5. training against the host call

def transitions(world, B, rng):
    idx = world.indices(B)
    b = world.rb.batch(idx, layout="nhwc_slot", fields=("s",))
    steps = []
    for _ in range(2):   # two successive updates on the same states with new actions and targets
        steps.append((rng.integers(0, 3, B).astype(np.uint8), rng.standard_normal(B).astype(np.float32)))
    return idx, b.s, steps


@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("B", [1, 33, 64])
def test_train_equals_host_call(world, arch, B):
    idx, s, steps = transitions(world, B, np.random.default_rng(100 + B))
    s_host = host(s)
    ref = qlx.DeepQLearningModel(seed=5, precision=PREC[arch])
    by_obs, by_replay, weighted, by_time, by_time_replay = (net(arch, seed=5) for _ in range(5))
    ones = torch.ones(B, device=DEV)
    s_time = world.rb.batch(idx, layout="nchw_time", fields=("s",)).s
    for a, y in steps:
        loss_ref = np.float32(ref.train(s_host, a, y))
        ad, yd = dev(a), dev(y)
        l1, td1 = by_obs.train(ad, yd, obs=s, layout="nhwc_slot", want_td_abs=True)
        l2, td2 = by_replay.train(ad, yd, replay=world.rb, indices=idx, layout="nhwc_slot", want_td_abs=True)
        l3, td3 = weighted.train(ad, yd, ones, obs=s, layout="nhwc_slot")
        l4, _ = by_time.train(ad, yd, obs=s_time, layout="nchw_time")
        l5, _ = by_time_replay.train(ad, yd, replay=world.rb, indices=idx, layout="nchw_time")
        assert same(host(l4), host(l5)), "the other channel convention: dense and replay source"
        assert td3 is None and l1.shape == ()
        for l in (l1, l2, l3):
            assert same(host(l), loss_ref)
        assert same(host(td1), host(td2)), "td_abs: dense and replay source"
    want = model_state(ref)
    assert want[1] == 2
    for m in (by_obs, by_replay, weighted):
        m.sync()
        assert same_state(model_state(m.model), want)
    by_time.sync(), by_time_replay.sync()
    assert same_state(model_state(by_time.model), model_state(by_time_replay.model))
    for m in (by_obs, by_replay, weighted, by_time, by_time_replay):
        m.close()
    ref.close()


def test_td_abs_is_q_minus_y_f32(world):
    """fp32: the forward is one fmaf chain per element whatever the batch, so |q[a] - y| from q() on the same batch before
    the update, one fp32 subtraction, is the td_abs the update reports"""
    B = 33
    idx, s, steps = transitions(world, B, np.random.default_rng(7))
    m = net("f32", seed=9)
    for a, y in steps:
        q = host(m.q(s, layout="nhwc_slot", want="q"))
        _, td = m.train(dev(a), dev(y), obs=s, layout="nhwc_slot", want_td_abs=True)
        want = np.abs(q[np.arange(B), a] - y).astype(np.float32)
        got = host(td)
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, [(int(i), float(got[i]), float(want[i])) for i in bad[:4]]
    m.sync()
    m.close()


# ---------------------------------------------------------------- 6. pinned to the learner's own update (fp32)

def test_train_reproduces_learner_update():
    N, B = 8, 16
    L = qlx.SelfDrivingQLearner(qlx.Parameter(n_envs=N, batch_size=B, history_buffer_len=200, update_after_actions=N,
                                              flags=qlx.PER, max_steps_per_episode=45))
    L.prefill(4)
    L.sync()
    twin = net("f32", seed=77, reserve=B)
    for v in range(qlx.NUM_VARS):
        for w in range(3):
            twin.model.set(v, L.model.get(v, w), w)
    assert L.model.iterations() == twin.model.iterations() == 0
    L.vector_step()
    last = L.last()
    assert last["losses"].shape[0] == 1, "exactly one update"
    isw, _, _ = L.priorities()
    rb = QT.TorchReplay(handle=qlx.lib().qlx_learner_replay(L.h), n_envs=N, device=DEV)
    idx = dev(last["indices"][0].astype(np.int64))
    actions = rb.batch(idx, fields=("actions",)).actions
    loss, _ = twin.train(actions, dev(last["targets"][0]), dev(isw[0]), replay=rb, indices=idx, layout="nhwc_slot")
    twin.sync()
    rb.sync()
    assert same(host(loss), last["losses"][0]) and same(host(loss), np.float32(L.stats()["last_loss"]))
    assert same_state(model_state(twin.model), model_state(L.model))
    twin.close()
    rb.close()
    L.close()


# ---------------------------------------------------------------- 7. a bad action

@pytest.mark.parametrize("arch", ARCHS)
def test_bad_action_trains_as_zero_and_is_reported_once(world, arch):
    B = 33
    idx, s, steps = transitions(world, B, np.random.default_rng(3))
    a, y = steps[0]
    a0, a3 = a.copy(), a.copy()
    a0[4], a3[4] = 0, 3
    m, twin = net(arch, seed=6), net(arch, seed=6)
    l_twin, _ = twin.train(dev(a0), dev(y), obs=s, layout="nhwc_slot")
    l_bad, _ = m.train(dev(a3), dev(y), obs=s, layout="nhwc_slot")
    with pytest.raises(qlx.QlError, match="action"):
        m.sync()
    m.sync()
    twin.sync()
    assert same(host(l_bad), host(l_twin)) and same_state(model_state(m.model), model_state(twin.model))
    m.close()
    twin.close()


# ---------------------------------------------------------------- 8. reserve, weight copies

@pytest.mark.parametrize("arch", ARCHS)
def test_reserve_bounds_every_call(world, pool, arch):
    m, twin = net(arch, seed=8, reserve=16), net(arch, seed=8, reserve=16)
    before = model_state(m.model)
    x = dev(pool[:17])
    a, y = dev(np.zeros(17, np.uint8)), dev(np.ones(17, np.float32))
    with pytest.raises(ValueError, match="reserve"):
        m.q(x, layout="nhwc_slot")
    with pytest.raises(ValueError):
        m.train(a, y, obs=x, layout="nhwc_slot")
    # the C calls themselves: QLX_E_STATE, nothing launched
    src = qlx.StatesDev(obs=x.data_ptr(), layout=qlx.OBS_NHWC_SLOT)
    out = torch.zeros(17 * 3, device=DEV)
    L = qlx.lib()
    assert L.qlx_model_q_dev(m.h, C.byref(src), 17, out.data_ptr(), None, None) == -4 and b"reserve" in L.qlx_last_error()
    assert L.qlx_model_train_dev(m.h, C.byref(src), a.data_ptr(), y.data_ptr(), None, 17, None, None) == -4
    assert b"reserve" in L.qlx_last_error()
    m.sync()
    assert not host(out).any() and same_state(model_state(m.model), before)
    for net_ in (m, twin):
        net_.train(a[:16], y[:16], obs=x[:16], layout="nhwc_slot")
    m.sync(), twin.sync()
    assert same_state(model_state(m.model), model_state(twin.model)) and m.model.iterations() == 1
    m.close()
    twin.close()


@pytest.mark.parametrize("arch", ARCHS)
def test_copy_weights_from(fwd_nets, pool, arch):
    src, dst = fwd_nets[arch], net(arch, seed=31)
    x = dev(pool[:33])
    ref = host(src.q(x, layout="nhwc_slot", want="q"))
    assert not same(host(dst.q(x, layout="nhwc_slot", want="q")), ref)
    dst.copy_weights_from(src)
    assert same(host(dst.q(x, layout="nhwc_slot", want="q")), ref)
    assert same(host(src.q(x, layout="nhwc_slot", want="q")), ref)
    dst.sync(), src.sync()
    dst.close()


def test_wrapped_handle_and_argument_errors(pool):
    owner = qlx.DeepQLearningModel(seed=2)
    m = QT.TorchQNet(handle=owner.h, device=DEV, reserve=8)
    x = dev(pool[:4])
    q = host(m.q(x, layout="nhwc_slot", want="q"))
    assert same(q, owner.q_values(pool[:4])[0])
    m.close()
    assert owner.iterations() == 0   # still alive: the wrapper does not own it
    owner.close()
    m = net("f32", reserve=8)
    for bad in (dict(obs=x.cpu()), dict(obs=x.float()), dict(obs=x, layout="nchw_time"), dict(obs=x, layout="hwc"), dict(),
                dict(obs=x, env=object()), dict(obs=x, layout="nhwc_slot", which="next"),
                dict(obs=x, layout="nhwc_slot", want=("q", "v")), dict(obs=x, layout="nhwc_slot", want=())):
        with pytest.raises(ValueError):
            m.q(**bad)
    with pytest.raises(ValueError):
        m.train(dev(np.zeros(4, np.int64)), dev(np.zeros(4, np.float32)), obs=x, layout="nhwc_slot")
    with pytest.raises(ValueError):
        QT.TorchQNet("fp16")
    m.sync()
    m.close()
    with pytest.raises(qlx.QlError):
        m.q(x, layout="nhwc_slot")
