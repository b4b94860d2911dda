"""The update tail across entry points on one live model.

train leaves clip-norm partials behind that belong to its own gradient (bf16: the producers' fused slots; fp32: the
scheduled dense partials and their flags).  apply_gradient replaces the gradient from outside, so it must not use them,
and the next train must not see what apply_gradient left.  One model runs train, apply_gradient(g1, 1/3), train,
apply_gradient(g2, 1.0) at B = 37; g1 and g2 are gradients of another batch, times 2 and times 0.01.

fp32: every call equals the oracle's (ref.train, O.qnet32_apply) bit for bit.
bf16: every call equals, byte for byte, the same call on a fresh model with the live one's state (a fresh model's fused
slots are zero and its flags clear), and the norms apply_gradient returns are within 1e-5 of float64
sqrt(sum (g scale)^2) - a live and a fresh model could agree on a wrong value only by accident.
"""
import numpy as np
import pytest

import oracle as O
from test_gpu_qnet32 import _qlx, env_states, randomize, same
from test_gpu_qnet_bf16_shapes import bf16_model, bits, fresh_copy, states

pytestmark = pytest.mark.gpu

B = 37


def flat(grads):
    return np.concatenate([g.ravel() for g in grads]).astype(np.float32)


def test_fp32_train_and_apply_gradient_interleaved_match_oracle():
    m = _qlx().DeepQLearningModel(seed=7)
    ref = O.QNet(seed=7, f32=True)
    randomize(m, ref, 5)
    rng = np.random.default_rng(9)

    def batch(x):
        a = rng.integers(0, 3, B).astype(np.uint8)
        y = (ref.forward(x)[np.arange(B), a] + rng.normal(0, 1.5, B)).astype(np.float32)
        return x, a, y

    other = O.QNet(seed=7, f32=True)
    other.load_state_from(ref)
    g = flat(other.train(*batch(env_states(B, seed=55)))[1])
    g1, g2 = g * np.float32(2.0), g * np.float32(0.01)

    def state(tag):
        for v in range(10):
            for which in range(3):
                assert same(m.get(v, which), ref.get(v, which)), f"{tag}: var {v} slot {which}"

    def train(x, tag):
        x, a, y = batch(x)
        loss, grads, norms = m.train(x, a, y, want_grads=True)
        loss_r, grads_r, norms_r = ref.train(x, a, y)
        assert same(np.float32(loss), np.float32(loss_r)), (tag, loss, loss_r)
        for v in range(10):
            bad = np.flatnonzero(grads[v].ravel().view(np.uint32) != grads_r[v].ravel().view(np.uint32))
            assert bad.size == 0, f"{tag}: gradient of var {v}: {bad.size} of {grads[v].size} differ (first {bad[:5]})"
        assert same(norms, norms_r), (tag, norms, norms_r)
        state(tag)

    def apply(grad, scale, tag):
        want = O.qnet32_apply(ref, grad, np.float32(scale))
        got = m.apply_gradient(grad, scale)
        assert same(got, want), (tag, got, want)
        state(tag)
        return want

    train(env_states(B), "first train")
    n1 = apply(g1, 1.0 / 3.0, "apply_gradient(g1, 1/3)")
    train(env_states(B, seed=321), "second train")
    n2 = apply(g2, 1.0, "apply_gradient(g2, 1)")
    seen = np.stack([n1, n2])
    assert (seen > 1.0).any() and (seen < 1.0).any(), seen   # both sides of clip_by_norm
    assert m.iterations() == ref.iterations() == 4


def test_bf16_train_and_apply_gradient_interleaved_match_fresh_model(tmp_path):
    live, _ = bf16_model(13, 1)
    rng = np.random.default_rng(8)

    def batch(x):
        return x, rng.integers(0, 3, B).astype(np.uint8), rng.normal(0, 1.5, B).astype(np.float32)

    src, _ = bf16_model(13, 1)
    grads = src.train(*batch(states(B, 9)), want_grads=True)[1]
    g = flat(grads)
    sizes = np.cumsum([0] + [x.size for x in grads])
    calls = [("train", batch(states(B, 1))), ("apply", (g * np.float32(2.0), 1.0 / 3.0)),
             ("train", batch(states(B, 2))), ("apply", (g * np.float32(0.01), 1.0))]
    for step, (call, args) in enumerate(calls):
        tag = f"call {step} ({call})"
        fresh = fresh_copy(live, str(tmp_path / "state.qlx"))
        if call == "train":
            n1, n2 = live.train(*args, want_grads=True)[-1], fresh.train(*args, want_grads=True)[-1]
        else:
            grad, scale = args
            n1, n2 = live.apply_gradient(grad, scale), fresh.apply_gradient(grad, scale)
            for v in range(10):
                want = np.sqrt(((grad[sizes[v]:sizes[v + 1]].astype(np.float64) * np.float64(np.float32(scale))) ** 2).sum())
                print(f"{tag}: norm of var {v}: live {n1[v]} fresh {n2[v]} float64 {want}")
                assert abs(n1[v] - want) <= 1e-5 * want, f"{tag}: norm of var {v}: {n1[v]} vs {want}"
        assert np.array_equal(bits(n1), bits(n2)), f"{tag}: norms {n1} vs {n2}"
        for v in range(10):
            for which in range(3):
                assert np.array_equal(bits(live.get(v, which)), bits(fresh.get(v, which))), f"{tag}: var {v} slot {which}"
        assert live.iterations() == fresh.iterations() == step + 1
