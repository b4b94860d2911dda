"""bf16 Q-net: one live model across batch sizes, and the update tail (clip_by_norm + Adam + the bf16 operand re-pack).

Workspace / cache reuse: the workspace only grows, so after a large batch every later, smaller batch runs over stale
activation rows, stale weight-gradient slab rows, stale norm partial slots and a block map built for another B.  The
kernels are fixed-order, so a model with that history must produce the very bytes a fresh model with the same
weights, Adam slots and iteration count produces: Q, loss, all ten gradients, norms and w / m / v, no tolerance.

Update tail: adam_elem (q-learning_amd/csrc/qnet_bf16.hip) restated in numpy float32, one rounded operation per line
(tests/bf16_checks.py adam_step), from the returned raw gradients, the returned norms and w / m / v read before the step;
w / m / v after the step are equal bit for bit (measured: 0 of 3 x 1,685,667 elements unequal at every step; the device's
division and square root are correctly rounded.  Before adam_elem kept the compiler from contracting m + d (1 - beta1),
gc gc - v and v + s (1 - beta2) into FMAs, step 2 differed in 25 % of m, 15 % of v and 0.5 % of w).  At t > 1 the step
depends on the clip factor, which the first step (m / sqrt(v) = +-1) hides.  After the third step the element-wise forward checks of
tests/test_gpu_qnet_bf16_shapes.py pass with the updated master weights: the re-packed bf16 operand copies follow them.
The scaled path (apply_gradient: the data-parallel tail, norms from the k_sumsq ranges): norms within 1e-5 of float64
sqrt(sum (g scale)^2), and the same Adam restatement.
"""
import numpy as np
import pytest

import bf16_checks as C
from test_gpu_qnet_bf16_shapes import _qlx, bf16_model, bits, check_forward, fresh_copy, states

pytestmark = pytest.mark.gpu


def slots(m):
    return [[m.get(v, which) for which in range(3)] for v in range(10)]


def test_live_model_equals_fresh_model_bit_for_bit(tmp_path):
    live, _ = bf16_model(13, 1)
    dense = np.random.default_rng(300).integers(1, 256, size=(300, 84, 84, 4), dtype=np.uint8)
    # (call, batch): the last one (every batch larger than any trained before) also needs a block map with more tiles
    seq = [("q", dense), ("train", states(129, 1)), ("train", states(37, 2)), ("q", states(37, 3)), ("train", states(129, 4)),
           ("train", states(257, 5))]
    rng = np.random.default_rng(8)
    for step, (call, x) in enumerate(seq):
        B = x.shape[0]
        fresh = fresh_copy(live, str(tmp_path / "state.qlx"))
        if call == "q":
            (q1, a1), (q2, a2) = live.q_values(x), fresh.q_values(x)
            assert np.array_equal(bits(q1), bits(q2)) and np.array_equal(a1, a2), f"step {step}: Q at B = {B}"
            continue
        a = rng.integers(0, 3, B).astype(np.uint8)
        y = rng.normal(0, 1.5, B).astype(np.float32)
        (l1, g1, n1), (l2, g2, n2) = live.train(x, a, y, want_grads=True), fresh.train(x, a, y, want_grads=True)
        assert np.float32(l1).view(np.uint32) == np.float32(l2).view(np.uint32), f"step {step}: loss at B = {B}: {l1} vs {l2}"
        for v in range(10):
            bad = np.flatnonzero(bits(g1[v]).ravel() != bits(g2[v]).ravel())
            assert bad.size == 0, f"step {step}, B = {B}: gradient of var {v}: {bad.size} elements differ, first {bad[:5]}"
        assert np.array_equal(bits(n1), bits(n2)), f"step {step}: norms at B = {B}: {n1} vs {n2}"
        for v, (s1, s2) in enumerate(zip(slots(live), slots(fresh))):
            for which in range(3):
                assert np.array_equal(bits(s1[which]), bits(s2[which])), f"step {step}, B = {B}: var {v} slot {which}"
        assert live.iterations() == fresh.iterations()


def check_adam(m, before, grads, norms, hp, t, scale, tag):
    unequal, total, report = 0, 0, []
    for v in range(10):
        want = C.adam_step(grads[v], norms[v], *before[v], hp, t, scale)
        for which in range(3):
            got = m.get(v, which)
            n = int((bits(got) != bits(want[which])).sum())
            unequal, total = unequal + n, total + got.size
            if n:
                report.append(f"var {v} {'wmv'[which]}: {n} of {got.size}")
    assert not report, f"{tag}: elements that differ from the float32 restatement: " + "; ".join(report)
    return unequal / total


def test_update_tail_three_steps():
    B = 37
    m, _ = bf16_model(31, 5)
    hp = _qlx().model_hparams()
    x = states(B, 9)
    rng = np.random.default_rng(77)
    a = rng.integers(0, 3, B).astype(np.uint8)
    seen = []
    for t in range(1, 4):
        y = rng.normal(0, 4.0 * t, B).astype(np.float32)
        before = slots(m)
        _, grads, norms = m.train(x, a, y, want_grads=True)
        seen.append(norms)
        share = check_adam(m, before, grads, norms, hp, t, 1.0, f"step {t}")
        print(f"step {t}: norms {norms}, share of w / m / v elements unequal to the restatement {share:.1e}")
    seen = np.array(seen)
    assert (seen > 1.0).any() and (seen < 1.0).any(), seen   # both sides of clip_by_norm
    assert m.iterations() == 3
    check_forward(m, m.weights(), x, "after 3 updates")   # the bf16 operand copies follow the updated masters


@pytest.mark.parametrize("scale", [1.0, 1.0 / 3.0, 1.0 / 8.0])
def test_scaled_update_tail(scale):
    B = 37
    src, _ = bf16_model(31, 5)
    rng = np.random.default_rng(78)
    x, a, y = states(B, 9), rng.integers(0, 3, B).astype(np.uint8), rng.normal(0, 4.0, B).astype(np.float32)
    _, grads, _ = src.train(x, a, y, want_grads=True)
    flat = np.concatenate([g.ravel() for g in grads]).astype(np.float32)
    m, _ = bf16_model(31, 5)
    hp = _qlx().model_hparams()
    sizes = np.cumsum([0] + [g.size for g in grads])
    seen = []
    for t in range(1, 3):
        g = flat * np.float32(0.01 if t == 2 else 1.0)   # the second gradient mostly below the clip norm
        before = slots(m)
        norms = m.apply_gradient(g, scale)
        seen.append(norms)
        parts = [g[sizes[v]:sizes[v + 1]].reshape(grads[v].shape) for v in range(10)]
        for v in range(10):
            want = np.sqrt(((parts[v].astype(np.float64) * np.float64(np.float32(scale))) ** 2).sum())
            assert abs(norms[v] - want) <= 1e-5 * want, f"t = {t}: norm of var {v}: {norms[v]} vs {want}"
        check_adam(m, before, parts, norms, hp, t, np.float32(scale), f"scale {scale:.3f} step {t}")
    seen = np.array(seen)
    assert (seen > 1.0).any() and (seen < 1.0).any(), seen
    assert m.iterations() == 2
