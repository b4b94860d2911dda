"""fp32 Q-net: one live model across batch sizes and frame kinds stays bit-equal to the oracle.

The fp32 workspace only grows too, and its background classification (C1Lists), chunk tables and row flags are rebuilt per
call inside it.  A 300-sample forward of background-free frames, then an update on 37 mostly-background env frames, then a
129-sample forward of single-pixel frames, then another update at 37: every Q, loss, gradient, norm and w / m / v equals
the oracle's (oracle/qnet32_ref.cpp) bit for bit, as tests/test_gpu_qnet32.py asserts of fresh models.
"""
import numpy as np
import pytest

import oracle as O
from test_gpu_qnet32 import _qlx, edge_states, env_states, randomize, same

pytestmark = pytest.mark.gpu


def test_live_fp32_model_stays_bit_exact():
    m = _qlx().DeepQLearningModel(seed=7)
    ref = O.QNet(seed=7, f32=True)
    randomize(m, ref, 5)
    rng = np.random.default_rng(9)

    def forward(x, tag):
        q, a = m.q_values(x)
        qr = ref.forward(x)
        assert same(q, qr), tag
        assert np.array_equal(a, np.argmax(qr, axis=1)), tag

    def train(x, tag):
        B = x.shape[0]
        a = rng.integers(0, 3, B).astype(np.uint8)
        y = (ref.forward(x)[np.arange(B), a] + rng.normal(0, 1.5, B)).astype(np.float32)
        loss, grads, norms = m.train(x, a, y, want_grads=True)
        loss_r, grads_r, norms_r = ref.train(x, a, y)
        assert same(np.float32(loss), np.float32(loss_r)), (tag, loss, loss_r)
        for v in range(10):
            bad = np.flatnonzero(grads[v].ravel().view(np.uint32) != grads_r[v].ravel().view(np.uint32))
            assert bad.size == 0, f"{tag}: gradient of var {v}: {bad.size} of {grads[v].size} differ (first {bad[:5]})"
        assert same(norms, norms_r), tag
        for v in range(10):
            for which in range(3):
                assert same(m.get(v, which), ref.get(v, which)), f"{tag}: var {v} slot {which} after Adam"

    forward(np.random.default_rng(300).integers(1, 256, size=(300, 84, 84, 4), dtype=np.uint8), "300 background-free frames")
    train(env_states(37), "first update at 37")
    forward(edge_states(129), "129 single-pixel frames")
    train(env_states(37, seed=321), "second update at 37")
    assert m.iterations() == ref.iterations() == 2
