"""Prioritized replay on device tensors (include/qlx.h) through qlx_torch on the GPU.  Everything is bit for
bit: leaves, per_max and the tree against the numpy restatement (per_reference.py), the tree's own invariant
t[i] == t[2i] + t[2i + 1], the draws and weights against the oracle sampler over the same leaves and against the learner's
k_per_sample (qlx.SumTree) - the new kernels against the old.  No tolerance, no case left out."""
import numpy as np
import pytest
import torch

import qlx_torch as QT   # before any other use of qlx in this process (it checks that itself)
import qlx
import oracle as O
import per_reference as P

pytestmark = pytest.mark.gpu

SEED = 0x51A5EED
DEV = "cuda:0"
BATCHES = (1, 5, 64, 67, 1024, 4096)
ALPHA, EPS = 0.6, 1e-6


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


class Ring:
    """a TorchEnv stepped with fixed actions into a TorchReplay, and the restatement fed the same pushes"""

    def __init__(self, cap, n_envs):
        self.cap, self.n = cap, n_envs
        self.env = QT.TorchEnv(n_envs, SEED, DEV)
        self.rb = QT.TorchReplay(cap, self.env)
        self.actions = dev((np.arange(n_envs) % 3).astype(np.uint8))
        self.ref = None

    def push(self, times=1):
        for _ in range(times):
            r, d = self.env.step(self.actions)
            self.rb.add(self.env, self.actions, r, d)
            if self.ref is not None:
                self.ref.push(self.n)

    def enable(self):
        self.rb.enable_priorities()
        self.ref = P.PerRef(self.cap, total=len(self.rb) if self.ref is None else self.ref.total)

    def close(self):
        self.env.close()


def check_state(ring, what):
    """leaves, tree invariant at every inner node, total, per_max and start"""
    rb, ref = ring.rb, ring.ref
    p = rb.priorities()
    t, cap = p["tree"], ring.cap
    L = t.shape[0] // 2
    assert L == P.leaves_pow2(cap), what
    assert same(p["leaves"], ref.leaves), f"leaves {what}"
    assert same(t[L:L + cap], ref.leaves) and not t[L + cap:].any(), f"tree leaves {what}"
    w = L >> 1
    while w >= 1:
        assert same(t[w:2 * w], t[2 * w:4 * w:2] + t[2 * w + 1:4 * w:2]), f"t[i] == t[2i] + t[2i+1] at width {w} {what}"
        w >>= 1
    assert p["per_max"] == ref.per_max and p["start"] == ref.start, what
    if ref.len:
        _, _, total = O.per_sample(ref.leaves, 1, 0, 1, 0, ref.len, 0.4, 1)
        assert p["total"] == np.float32(total) and (L == 1 or t[1] == p["total"]), f"total {what}"
    assert len(rb) == ref.len


def spread_update(ring, rng, calls=2):
    """priorities with a wide spread (gamma-distributed |td|, as test_gpu_per.py's leaves), through update_priorities"""
    ref = ring.ref
    for _ in range(calls):
        n = int(min(4096, max(1, ref.len)))
        idx = rng.integers(0, ref.len, n).astype(np.int64)
        td = rng.gamma(0.4, 1.0, n).astype(np.float32)
        ring.rb.update_priorities(dev(idx), dev(td), ALPHA, EPS)
        assert not ref.update(idx, td, ALPHA, EPS)


def check_draws(ring, what):
    rb, ref = ring.rb, ring.ref
    old = qlx.SumTree(ring.cap)
    old.set_leaves(ref.leaves)
    for k, B in enumerate(BATCHES):
        for beta in ((0.4, 0.0) if B in (67, 4096) else (0.4,)):
            upd, rank = 17 + k, k % 3
            idx, w = rb.sample_prioritized(B, SEED, upd, beta, rank)
            idx, w = idx.cpu().numpy(), w.cpu().numpy()
            assert idx.dtype == np.int64 and w.dtype == np.float32
            r_idx, r_w, _ = ref.sample(SEED, upd, rank, beta, B)
            assert same(idx.view(np.uint64), r_idx), f"indices vs oracle, B={B} beta={beta} {what}"
            assert same(w, r_w), f"weights vs oracle, B={B} beta={beta} {what}"
            o_slots, o_w = old.sample(SEED, upd, 1, rank, ref.len, beta, B)
            assert same(idx.view(np.uint64), ref.to_logical(o_slots[0])), f"indices vs k_per_sample, B={B} {what}"
            assert same(w, o_w[0]), f"weights vs k_per_sample, B={B} {what}"
            if beta == 0.0:
                assert (w == 1.0).all()
    old.close()


# capacity, n_envs: L = 2; L = 4; -; a push wraps mid-call; the largest single-block tree; L = 4096, the first with two
# build launches; -; L = 2^17; L = 2^19.  log2 L mod 3 = 1, 2, 0, 1, 2, 0, 1, 2, 1: every tail of the three-level descent
SHAPES = [(2, 1), (3, 1), (8, 2), (100, 8), (2048, 64), (2049, 64), (5000, 8), (70_000, 1024), (270_000, 8192)]


@pytest.mark.parametrize("cap,n_envs", SHAPES)
def test_tree_and_draws_before_and_after_the_wrap(cap, n_envs):
    rng = np.random.default_rng(cap)
    ring = Ring(cap, n_envs)
    fill = -(-cap // n_envs)              # pushes until len == cap
    ring.push(max(1, fill // 2))
    assert 0 < len(ring.rb) < cap
    ring.enable()
    check_state(ring, "after enable")
    spread_update(ring, rng)
    check_state(ring, "after updates, len < cap")
    check_draws(ring, "len < cap")        # slots >= len are empty subtrees: the right == 0 rule
    while ring.ref.total < cap + n_envs or ring.ref.start == 0:
        ring.push()
        check_state(ring, f"after push {ring.ref.total // n_envs}")
    assert len(ring.rb) == cap and ring.ref.start != 0
    spread_update(ring, rng, calls=3)
    check_state(ring, "after updates, wrapped")
    check_draws(ring, "wrapped")
    ring.push()
    check_state(ring, "after a push on the wrapped ring")
    ring.rb.enable_priorities()           # a second enable resets to priority 1
    ring.ref = P.PerRef(cap, total=ring.ref.total)
    check_state(ring, "after a second enable")
    ring.rb.sync()
    ring.close()


def test_updates_last_writer_guards_and_empty():
    cap, n = 1000, 8
    ring = Ring(cap, n)
    ring.push(40)                          # len 320
    ring.enable()
    rng = np.random.default_rng(5)
    idx = rng.integers(0, 50, 400).astype(np.int64)   # 400 writes over 50 slots: many repeats
    td = (rng.random(400) * 3).astype(np.float32)
    ring.rb.update_priorities(dev(idx), dev(td), ALPHA, EPS)
    assert not ring.ref.update(idx, td, ALPHA, EPS)
    pr = O.det_powf(td + np.float32(EPS), ALPHA)
    last = {int(i): k for k, i in enumerate(idx)}
    assert all(ring.ref.leaves[i] == pr[k] for i, k in last.items())
    check_state(ring, "after 400 writes over 50 slots")
    ring.rb.sync()

    # entries the host cannot see: index >= len (320, cap, -1), td_abs NaN, +inf, -1; the valid ones are written
    before = ring.rb.priorities()
    idx = np.array([3, 320, 7, cap, -1, 11, 12, 13, 200, 3], np.int64)
    td = np.array([5.0, 1.0, np.nan, 1.0, 1.0, np.inf, -1.0, 0.0, 2.5, 0.25], np.float32)
    ring.rb.update_priorities(dev(idx), dev(td), ALPHA, EPS)
    with np.errstate(invalid="ignore"):
        assert ring.ref.update(idx, td, ALPHA, EPS)
    after = ring.rb.priorities()
    for slot in (7, 11, 12):
        assert after["leaves"][slot] == before["leaves"][slot]
    assert after["leaves"][13] == O.det_powf(np.float32(EPS), ALPHA)[()]
    assert after["leaves"][3] == O.det_powf(np.float32(0.25) + np.float32(EPS), ALPHA)[()]   # the last valid writer
    assert after["leaves"][200] == O.det_powf(np.float32(2.5) + np.float32(EPS), ALPHA)[()]
    assert not after["leaves"][320:].any()
    assert after["per_max"] == max(before["per_max"], O.det_powf(np.float32(5.0) + np.float32(EPS), ALPHA)[()])
    assert np.isfinite(after["tree"]).all()
    check_state(ring, "after a batch with refused entries")
    with pytest.raises(qlx.QlError, match="out of range"):
        ring.rb.sync()
    ring.rb.sync()   # reported once

    # only refused entries: nothing changes, per_max included
    ring.rb.update_priorities(dev(np.array([0, 1], np.int64)), dev(np.array([np.inf, np.nan], np.float32)))
    assert same(ring.rb.priorities()["tree"], after["tree"]) and ring.rb.priorities()["per_max"] == after["per_max"]
    with pytest.raises(qlx.QlError):
        ring.rb.sync()

    # n = 0 is a no-op
    ring.rb.update_priorities(torch.empty(0, dtype=torch.int64, device=DEV), torch.empty(0, dtype=torch.float32, device=DEV))
    assert same(ring.rb.priorities()["tree"], after["tree"])
    ring.rb.sync()
    with pytest.raises(ValueError):
        ring.rb.update_priorities(dev(idx[:4]), dev(td[:3]))
    ring.close()


def test_off_means_off():
    """Two replays fed the same steps, one with priorities: the one without refuses the prioritized calls, and its pushes,
    uniform samples and batches are the other's."""
    n, cap = 4, 50
    env = QT.TorchEnv(n, SEED, DEV)
    plain, prio = QT.TorchReplay(cap, env), QT.TorchReplay(cap, env)
    prio.enable_priorities()   # on an empty replay
    a = dev(np.array([0, 1, 2, 1], np.uint8))
    for t in range(15):   # 60 pushes: wrapped
        r, d = env.step(a)
        plain.add(env, a, r, d)
        prio.add(env, a, r, d)
    idx = torch.arange(4, dtype=torch.int64, device=DEV)
    td = torch.ones(4, device=DEV)
    for call in (lambda: plain.sample_prioritized(8, SEED, 0), lambda: plain.update_priorities(idx, td),
                 lambda: plain.priorities()):
        with pytest.raises(qlx.QlError, match="not enabled"):
            call()
    prio.update_priorities(idx, td * 3)
    assert len(plain) == len(prio) == cap
    for u in range(3):
        i0, i1 = plain.sample_indices(16, SEED, u), prio.sample_indices(16, SEED, u)
        assert same(i0.cpu().numpy(), i1.cpu().numpy())
        b0, b1 = plain.batch(i0, n_step=3), prio.batch(i1, n_step=3)
        for x, y in zip(tuple(b0) + (b0.last_indices,), tuple(b1) + (b1.last_indices,)):
            assert same(x.cpu().numpy(), y.cpu().numpy())
    p = prio.priorities()
    assert p["start"] == 10 and (p["leaves"] > 0).all()
    plain.sync()
    prio.sync()
    env.close()


def test_loop_with_the_qnet_and_a_single_sync():
    """sample -> batch -> targets in torch -> TorchQNet.train(weights, want_td_abs) -> update_priorities -> step + add, a
    dozen times with nothing read back; then one sync, and the recorded indices and |td| replayed through the restatement
    give every draw and the final leaves."""
    n, cap, B, beta = 16, 512, 32, 0.4
    ring = Ring(cap, n)
    net = QT.TorchQNet("f32", seed=2, env=ring.env, reserve=B)
    ring.push(26)    # len 416; the ring wraps during the loop
    ring.rb.enable_priorities()
    total0 = len(ring.rb)
    rec = []
    for it in range(12):
        idx, w = ring.rb.sample_prioritized(B, SEED, it, beta)
        b = ring.rb.batch(idx, fields=("actions", "returns", "discounts", "terminals", "last_indices"))
        q_next = net.q(replay=ring.rb, indices=b.last_indices, which="s_next", want="max_q")
        y = b.returns + b.discounts * q_next * (1.0 - b.terminals.float())
        _, td = net.train(b.actions, y, w, replay=ring.rb, indices=idx, want_td_abs=True)
        ring.rb.update_priorities(idx, td, ALPHA, EPS)
        rec.append((idx, w, td))
        ring.push()
    torch.cuda.synchronize()
    ring.env.sync()
    ring.rb.sync()
    net.sync()
    ref = P.PerRef(cap, total=total0)
    for it, (idx, w, td) in enumerate(rec):
        idx, w, td = idx.cpu().numpy(), w.cpu().numpy(), td.cpu().numpy()
        r_idx, r_w, _ = ref.sample(SEED, it, 0, beta, B)
        assert same(idx.view(np.uint64), r_idx) and same(w, r_w), f"draw {it}"
        assert np.isfinite(td).all() and not ref.update(idx, td, ALPHA, EPS)
        ref.push(n)
    assert ref.start != 0 and (ref.leaves != 1.0).any()
    ring.ref = ref
    check_state(ring, "after the loop")
    ring.close()
