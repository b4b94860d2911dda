"""The device-tensor env / replay calls through qlx_torch on the GPU (include/qlx.h), byte for byte against
the host calls they stand beside (qlx_env_obs, qlx_replay_get_many, qlx_replay_nstep, qlx_replay_sample_distinct) and, for
NCHW_TIME, the numpy restatement in obs_layout_reference.py.  Nothing here has a tolerance: states are bytes and the n-step
sums are replay_nstep's own fp32 operations."""
import ctypes

import numpy as np
import pytest
import torch

import obs_layout_reference as R
import qlx_torch as QT   # before any other use of qlx in this process (it checks that itself)
import qlx

pytestmark = pytest.mark.gpu

SEED = 0x51A5EED
GAMMA = 0.99
DEV = "cuda:0"


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def host(t):
    return None if t is None else t.cpu().numpy()


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


# ---------------------------------------------------------------- env

def test_env_obs_step_reset_against_host_twin():
    n = 5
    te = QT.TorchEnv(n, SEED, DEV)
    twin = qlx.BreakoutEnvironment(n, SEED)
    rng = np.random.default_rng(3)
    observed = []
    for t in range(7):
        if t in (0, 1, 3, 4, 6):
            ref = twin.state()
            ns = twin.mechanics()["next_slot"]
            assert same(host(te.obs("nhwc_slot")), ref), f"NHWC_SLOT after {t} steps"
            assert same(host(te.obs("nchw_time")), R.env_nchw_time(ref, ns)), f"NCHW_TIME after {t} steps"
            assert same(te._env.state(), ref)
            observed.append(t)
        a = rng.integers(0, 3, n).astype(np.uint8)
        r, d = te.step(dev(a))
        _, r_ref, d_ref = twin.step(a)
        assert same(host(r), r_ref) and same(host(d).astype(bool), d_ref)
        if t == 2:   # after step 3: env 1 starts a new episode, so its older channels are zero frames again
            mask = np.array([0, 1, 0, 0, 0], np.uint8)
            te.reset(dev(mask))
            twin.reset(mask)
        assert same(te.mechanics(), twin.mechanics()) and same(te.hashes(), twin.hashes())
    assert observed == [0, 1, 3, 4, 6]
    out = torch.full((n, 4, 84, 84), 255, dtype=torch.uint8, device=DEV)
    assert te.obs("nchw_time", out=out) is out
    assert same(host(out), R.env_nchw_time(twin.state(), twin.mechanics()["next_slot"]))
    te.reset()
    twin.reset()
    assert same(te.mechanics(), twin.mechanics()) and not host(te.obs()).any()
    te.sync()


# ---------------------------------------------------------------- replay

N_ENVS, CAP, T = 3, 37, 20


class World:
    """3 envs, capacity 37, 20 vector steps = 60 pushes through device tensors: the ring wraps and 37 is no multiple of 3.
    Env 0 is given a done at step 10 and reset, env 1 is reset without a done after step 13, env 2 plays on: the live
    transitions (push positions 23 .. 59) have episode steps 1, 2, 3, ... of envs 0 and 1 and 8 .. 20 of env 2."""

    def __init__(self):
        self.env = QT.TorchEnv(N_ENVS, SEED, DEV)
        self.rb = QT.TorchReplay(CAP, self.env)
        rng = np.random.default_rng(17)
        ep = np.zeros(N_ENVS, np.int64)
        epstep = []
        for t in range(T):
            a = dev(rng.integers(0, 3, N_ENVS).astype(np.uint8))
            _, d = self.env.step(a)
            rewards = dev(rng.standard_normal(N_ENVS).astype(np.float32))   # stored as given: makes the sums non-trivial
            cut = np.zeros(N_ENVS, np.uint8)
            if t == 9:
                d = d | dev(np.array([1, 0, 0], np.uint8))
                cut[0] = 1
            if t == 12:
                cut[1] = 1
            self.rb.add(self.env, a, rewards, d)
            ep += 1
            epstep.extend(ep)
            if cut.any():
                self.env.reset(dev(cut))
                ep[cut != 0] = 0
        self.rb.sync()
        assert len(self.rb) == CAP
        self.epstep = np.array(epstep[T * N_ENVS - CAP:], np.int64)   # by logical index
        self.hostrb = self.rb._rb                                     # the host calls on the same handle
        self._ref = {}

    def indices(self, B):
        if B == 1:
            return np.array([30], np.uint64)
        if B == 5:
            return np.array([36, 0, 7, 8, 22], np.uint64)
        return (np.arange(B, dtype=np.uint64) * 7 + 3) % CAP   # 64 and 67: every live index, some twice

    def reference(self, B, n_step):
        """the host calls at indices(B), computed once per (B, n_step) and never written to"""
        key = (B, n_step)
        if key not in self._ref:
            idx = self.indices(B)
            g = self.hostrb.get_many(idx)
            w = self.hostrb.nstep(idx, n_step, GAMMA)
            nxt = self.hostrb.get_many(w["last_indices"])["state_next"]
            ref = dict(idx=idx, s=g["state"], s_next=nxt, actions=g["action"], returns=w["returns"], discounts=w["discounts"],
                       terminals=w["terminals"].astype(np.uint8), last_indices=w["last_indices"], steps=w["steps"])
            ref["s_time"] = R.replay_nchw_time(ref["s"], self.epstep[idx.astype(np.int64)], False)
            ref["s_next_time"] = R.replay_nchw_time(nxt, self.epstep[w["last_indices"].astype(np.int64)], True)
            for v in ref.values():
                v.setflags(write=False)
            self._ref[key] = ref
        return self._ref[key]


@pytest.fixture(scope="module")
def world():
    return World()


def check_batch(got, ref, layout, fields=QT._FIELDS):
    time = layout == "nchw_time"
    want = dict(ref, s=ref["s_time"] if time else ref["s"], s_next=ref["s_next_time"] if time else ref["s_next"])
    have = dict(s=got.s, s_next=got.s_next, actions=got.actions, returns=got.returns, discounts=got.discounts,
                terminals=got.terminals, last_indices=got.last_indices, steps=got.steps)
    for k in QT._FIELDS:
        if k not in fields:
            assert have[k] is None, k
            continue
        g = host(have[k])
        if k == "last_indices":
            g = g.astype(np.uint64)
        if k == "steps":
            g = g.astype(np.uint32)
        assert same(g, want[k]), f"{k} differs ({layout})"
    assert same(host(got.indices).astype(np.uint64), ref["idx"])


def test_world_reaches_every_edge(world):
    k = world.epstep
    assert {1, 2, 3} <= set(k.tolist()) and (k >= 5).any()
    ref = world.reference(64, 3)
    assert set(ref["idx"].tolist()) == set(range(CAP))
    short = ref["steps"] < 3
    edge = ref["last_indices"] + N_ENVS >= CAP
    assert (short & (ref["terminals"] != 0)).any(), "a window ended by a done"
    assert (short & (ref["terminals"] == 0) & ~edge).any(), "a window ended by a reset without a done"
    assert (short & edge).any(), "a window ended at the newest transition"
    assert not ref["s"][k[ref["idx"].astype(np.int64)] == 1].any(), "s of an episode's first transition is all zero frames"


@pytest.mark.parametrize("layout", ["nhwc_slot", "nchw_time"])
@pytest.mark.parametrize("n_step", [1, 3])
@pytest.mark.parametrize("B", [1, 5, 64, 67])
def test_batch_matches_host_calls(world, B, n_step, layout):
    ref = world.reference(B, n_step)
    got = world.rb.batch(dev(ref["idx"].astype(np.int64)), n_step, GAMMA, layout)
    check_batch(got, ref, layout)
    world.rb.sync()


@pytest.mark.parametrize("fields", [("s",), ("s_next", "returns"), ("actions", "steps"), ("s", "terminals", "last_indices")])
@pytest.mark.parametrize("layout", ["nhwc_slot", "nchw_time"])
def test_batch_with_null_outputs(world, layout, fields):
    ref = world.reference(67, 3)
    got = world.rb.batch(dev(ref["idx"].astype(np.int64)), 3, GAMMA, layout, fields=fields)
    check_batch(got, ref, layout, fields)


@pytest.mark.parametrize("B", [37, 5])
def test_sample_indices_match_host_sampler(world, B):
    for u in (0, 5):
        want = world.hostrb.sample_distinct(99, u, B, rank=1)
        got = host(world.rb.sample_indices(B, 99, u, rank=1))
        assert same(got.astype(np.uint64), want)
    b = world.rb.sample(B, 99, 5, n_step=3, gamma=GAMMA, rank=1)
    assert same(host(b.indices).astype(np.uint64), world.hostrb.sample_distinct(99, 5, B, rank=1))
    w = world.hostrb.nstep(host(b.indices).astype(np.uint64), 3, GAMMA)
    assert same(host(b.returns), w["returns"]) and same(host(b.last_indices).astype(np.uint64), w["last_indices"])
    with pytest.raises(ValueError):
        world.rb.sample_indices(CAP + 1, 99, 0)
    o = ctypes.c_void_p(0x1000)   # not dereferenced: the call fails on the host
    assert qlx.lib().qlx_replay_sample_distinct_dev(world.rb.h, 99, 0, 0, CAP + 1, o) == -1   # batch > len, from the ABI itself


@pytest.mark.parametrize("layout", ["nhwc_slot", "nchw_time"])
def test_index_out_of_range_is_guarded(world, layout):
    """one index >= len: that sample is the all-zero sample, its neighbours are untouched, sync() reports it once.  The
    kernel reads nothing for it (the guard comes before every load), so this provokes no fault."""
    world.rb.sync()
    ref = world.reference(5, 3)
    idx = ref["idx"].astype(np.int64).copy()
    bad = 2
    idx[bad] = 1000
    shape = (5, 4, 84, 84) if layout == "nchw_time" else (5, 84, 84, 4)
    out = dict(s=torch.full(shape, 255, dtype=torch.uint8, device=DEV), s_next=torch.full(shape, 255, dtype=torch.uint8, device=DEV),
               actions=torch.full((5,), 255, dtype=torch.uint8, device=DEV), returns=torch.full((5,), 7.0, device=DEV),
               discounts=torch.full((5,), 7.0, device=DEV), terminals=torch.full((5,), 255, dtype=torch.uint8, device=DEV),
               last_indices=torch.full((5,), -1, dtype=torch.int64, device=DEV), steps=torch.full((5,), -1, dtype=torch.int32, device=DEV))
    got = world.rb.batch(dev(idx), 3, GAMMA, layout, out=out)
    assert got.s is out["s"] and got.steps is out["steps"]
    time = layout == "nchw_time"
    want = dict(s=ref["s_time"] if time else ref["s"], s_next=ref["s_next_time"] if time else ref["s_next"])
    keep = np.arange(5) != bad
    for k in QT._FIELDS:
        g = host(out[k])
        w = want.get(k, ref[k])
        assert same(g[keep].astype(w.dtype), w[keep]), f"neighbours' {k}"
    assert not host(out["s"])[bad].any() and not host(out["s_next"])[bad].any()
    assert host(out["actions"])[bad] == 0 and host(out["returns"])[bad] == 0.0 and host(out["discounts"])[bad] == 0.0
    assert host(out["terminals"])[bad] == 1 and host(out["last_indices"])[bad] == 1000 and host(out["steps"])[bad] == 0
    with pytest.raises(qlx.QlError, match="out of range"):
        world.rb.sync()
    world.rb.sync()   # the flag was cleared
    # the states alone (no metadata launch) raise the flag too
    world.rb.batch(dev(idx), 1, GAMMA, layout, fields=("s",))
    with pytest.raises(qlx.QlError, match="out of range"):
        world.rb.sync()
    world.rb.sync()


# ---------------------------------------------------------------- stream order, arguments

def test_stream_order_against_torch_work():
    n = 5
    te = QT.TorchEnv(n, SEED, DEV)
    twin = qlx.BreakoutEnvironment(n, SEED)
    base = np.array([2, 0, 1, 2, 1], np.uint8)
    x = torch.ones((4096, 4096), device=DEV)
    for _ in range(3):
        y = x @ x                                  # a few ms of work on the current stream
    # the actions exist only once the matmul has run: every element of y is 4096
    a = (y[0, :n] / 4096 - 1 + dev(base, torch.float32)).to(torch.uint8)
    r, d = te.step(a)
    _, r_ref, d_ref = twin.step(base)
    assert same(host(a), base)
    assert same(host(r), r_ref) and same(te.mechanics(), twin.mechanics()) and same(te.hashes(), twin.hashes())
    # a result consumed at once by torch on its own stream
    total = te.obs("nchw_time").to(torch.int64).sum()
    assert int(total) == int(twin.state().astype(np.int64).sum()) and int(total) > 0


def test_argument_checks_come_before_any_launch():
    n = 8
    te = QT.TorchEnv(n, SEED, DEV)
    rb = QT.TorchReplay(16, te)
    a = torch.zeros(n, dtype=torch.uint8, device=DEV)
    r, d = te.step(a)
    rb.add(te, a, r, d)
    rb.sync()
    before = te.hashes()
    wide = torch.zeros(2 * n + 16, dtype=torch.uint8, device=DEV)
    bad_actions = [torch.zeros(n, dtype=torch.uint8),                       # on the CPU
                   torch.zeros(n, dtype=torch.int64, device=DEV),           # wrong dtype
                   wide[:2 * n:2],                                          # not contiguous
                   wide[4:4 + n],                                           # 4 bytes into an allocation
                   torch.zeros(n + 1, dtype=torch.uint8, device=DEV)]       # wrong shape
    for t in bad_actions:
        with pytest.raises(ValueError):
            te.step(t)
        with pytest.raises(ValueError):
            rb.add(te, t, r, d)
        with pytest.raises(ValueError):
            te.reset(t)
    buf = torch.zeros(n * 28224 + 16, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        te.obs("nchw_time", out=buf[4:4 + n * 28224].view(n, 4, 84, 84))
    with pytest.raises(ValueError):
        te.obs("nchw_time", out=torch.zeros((n, 84, 84, 4), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        te.obs("chw")
    idx = torch.zeros(4, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError):
        rb.batch(idx.cpu())
    with pytest.raises(ValueError):
        rb.batch(idx.to(torch.int32))
    with pytest.raises(ValueError):
        rb.batch(idx, n_step=0)
    with pytest.raises(ValueError):
        rb.batch(idx, out=dict(s=buf[4:4 + 4 * 28224].view(4, 4, 84, 84)))
    with pytest.raises(ValueError):
        rb.batch(idx, fields=("rewards",))
    te.sync()
    rb.sync()
    assert same(te.hashes(), before), "a refused call changed the env"
    assert len(rb) == n


def test_wrapping_a_learners_replay():
    """a learner's replay handle read through device tensors on the learner's stream"""
    L = qlx.SelfDrivingQLearner(qlx.Parameter(n_envs=4, batch_size=8, history_buffer_len=64, update_after_actions=4))
    L.prefill(6)
    L.sync()
    h = qlx.lib().qlx_learner_replay(L.h)
    rb = QT.TorchReplay(handle=h, n_envs=4, device=DEV)
    assert len(rb) == 24
    idx = np.array([0, 5, 23, 11], np.uint64)
    got = rb.batch(dev(idx.astype(np.int64)), 2, GAMMA, "nhwc_slot")
    g = rb._rb.get_many(idx)
    w = rb._rb.nstep(idx, 2, GAMMA)
    assert same(host(got.s), g["state"]) and same(host(got.actions), g["action"])
    assert same(host(got.returns), w["returns"]) and same(host(got.last_indices).astype(np.uint64), w["last_indices"])
    assert same(host(got.s_next), rb._rb.get_many(w["last_indices"])["state_next"])
    rb.sync()
