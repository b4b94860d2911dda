"""The float64 BallGame restatement (tests/ballgame_reference.py) held to the CPU oracle (oracle/ballgame_ref.cpp, fp32 with
float64 dot products) with the tolerances that tests/test_gpu_ballgame_shapes.py holds the HIP kernels to against the
restatement: Q rtol 1e-4 / atol 1e-5 max(1, max|q|), loss 1e-4 relative, gradients 1e-3 relative L2 per variable, norms
1e-3, weights after the Adam step 2e-7 (4e-7 after the second).  The reference alone stays inside them, so a GPU failure
is the kernel's.

Measured here, error / tolerance (B = 5 / 65; second step at 37 after 65): Q 1.5e-3 / 1.5e-3, loss 1.1e-4 / 1.4e-4,
gradients <= 1.2e-4, norms <= 6.5e-5, Adam 0.28 / 0.046 (the second step 0.037); only the Adam step uses a visible
part of its tolerance (its update is lr g / (|g| + 3.2e-6) at the first step, so a gradient error of 1e-9 at |g| ~ 1e-6
moves a weight by ~ 5e-8).
"""
import numpy as np
import pytest

import ballgame_reference as R
import oracle as O
from test_gpu_ballgame import rand_obs


def oracle_and_restatement(seed):
    ref = O.BgNet(seed=seed)
    w = R.nonzero_biases(ref.weights())
    for v in (1, 3, 5, 7):
        ref.set(v, w[v])
    return ref, R.Net(w, ref.hparams())


def step(ref, net, x, steps, tag):
    q = ref.forward(x)
    q64 = net.q_values(x)
    rq = R.q_ratio(q, q64)
    a, y = R.actions_and_targets(q64)
    before = [[ref.get(v, which) for v in range(8)] for which in range(3)]
    loss, g, nrm = ref.train(x, a, y)
    l64, g64, n64 = net.train(x, a, y)
    ratios = R.step_ratios(loss, g, nrm, ref.weights(), l64, g64, n64, net.w, steps)
    ratios["k_adam"] = R.own_adam_ratio(g, nrm, before, ref.weights(), net.hp, steps)   # the oracle's step: the same bits
    worst = max(ratios, key=ratios.get)
    print(f"{tag}: Q error / tolerance {rq:.2e}; worst of the step {worst} {ratios[worst]:.2e}; "
          f"loss {ratios['loss']:.2e}, gradients {max(ratios[f'grad{v}'] for v in range(8)):.2e}, "
          f"norms {max(ratios[f'norm{v}'] for v in range(8)):.2e}, adam {max(ratios[f'adam{v}'] for v in range(8)):.2e}, "
          f"the oracle's Adam on its own gradients {ratios['k_adam']:.2e}")
    assert rq <= 1.0
    d = R.decided_rows(q64)
    assert np.array_equal(q.argmax(axis=1)[d], q64.argmax(axis=1)[d])
    assert all(r <= 1.0 for r in ratios.values()), {k: r for k, r in ratios.items() if r > 1.0}


@pytest.mark.parametrize("B", [5, 65])
def test_restatement_matches_oracle(B):
    ref, net = oracle_and_restatement(5)
    step(ref, net, rand_obs(B, 9), 1, f"B={B}")
    assert net.iterations == 1


def test_restatement_matches_oracle_over_two_steps():
    ref, net = oracle_and_restatement(5)
    step(ref, net, rand_obs(65, 9), 1, "B=65")
    step(ref, net, rand_obs(37, 10), 2, "then B=37")


def test_same_padding_is_trailing():
    """A kernel tap at (1, 1) reads the zero padding at i = 2 or j = 2, never data before (0, 0)."""
    w = [np.zeros(s, np.float32) for s in R.VAR_SHAPES]
    w[0][1, 1, :, 0] = 1.0
    x = np.zeros((1, 3, 3, 4), np.uint8)
    x[0, :, :, 0] = 1
    a1 = R.forward(w, x)["a1"][0, :, :, 0]
    assert np.array_equal(a1, [[1, 1, 0], [1, 1, 0], [0, 0, 0]])
