"""BallGame Q-model kernels (q-learning_amd/csrc/ballgame.hip: k_conv_fwd, k_gemm_f32<TA, TB, EPI>, k_head<MODE>, k_colsum,
k_conv1_wgrad, k_norms, k_adam) at ragged batches against the float64 restatement (tests/ballgame_reference.py, which
tests/test_ballgame_reference.py holds to the CPU oracle with the same tolerances).

tests/test_gpu_ballgame.py checks values at B = 512 (the learners run 64 and 256): multiples of the 64 x 64 gemm tile, of
its 16-wide k step, of the head's 4 samples per block and of the 4 / 8 row phases of k_colsum / k_conv1_wgrad.  Each B
here with what it is the smallest shape to reach:
    1    one row in the only gemm tile; k_colsum with 1 row over 4 phases; k_conv1_wgrad with 9 rows over 8 phases; a head
         block with three idle waves; weight-gradient gemms with K = 1 and K = 9, below the k step
    3, 5 B % 4 != 0 in the head; K = 27 and 45: ragged k steps
    63   one row short of a full M tile
    65   a second M tile holding one row, in the forward (EPI 1) and in both masked backward-data gemms (EPI 2 reads
         aux[m ldc + n] at that row); K = 65 = 4 * 16 + 1
    100  a ragged second tile; K = 900 in the conv weight gradients
Non-zero biases, the observations, actions (arange(B) % 5) and targets (y = q_ref[a] + sin(arange(B))) of
tests/test_gpu_ballgame.py; at B = 1 the target is q_ref[a] + sin(1) (ballgame_reference.actions_and_targets says why).

Tolerances, those tests/test_gpu_ballgame.py states and justifies, as error / tolerance ratios (<= 1 passes):
    Q against float64 rtol 1e-4, atol 1e-5 max(1, max|q|); argmax equal wherever the reference's top-2 margin exceeds twice
    that; batch_predict_max_future_reward bit-equal to q.max(axis=1) of the returned Q; loss 1e-4 relative; every variable's
    gradient 1e-3 relative L2; every norm 1e-3; after the step's Adam |w - w_ref| <= 2e-7 (4e-7 after a second step);
    iterations() == 1.
At these sizes one dropped sample or k row moves a gradient by at least about 1 / B >= 1e-2 of its norm.

Bit for bit: k_gemm_f32's k order per output does not depend on m0 and every other forward kernel works per sample, so
q(x[perm]) == q(x)[perm] at B = 100 and samples 0, 63, 64, 99 alone at B = 1 equal their rows at B = 100.

A second train on the same model at a smaller batch (100 then 37; B <= ws_batch keeps the larger buffers) against the
restatement carried through both steps: no stale row of the first batch reaches k_colsum or the weight-gradient gemms.

k_adam is also checked alone (ballgame_reference.own_adam_ratio): the restated step on the product's own gradients, norms
and slots against the product's weights, within one rounding of w (bound derived there).

Measured on the MI355X, error / tolerance, worst per B = 1, 3, 5, 63, 65, 100 (then 37 as the second step after 100):
    Q          3.1e-4, 1.5e-3, 1.5e-3, 1.5e-3, 1.5e-3, 1.5e-3 (1.2e-3)
    loss       7.0e-5, 2.0e-4, 1.1e-4, 4.3e-4, 1.4e-4, 1.4e-4 (3.4e-5)
    gradients  6.9e-5, 7.6e-5, 6.8e-5, 1.2e-4, 1.1e-4, 3.8e-4 (1.0e-4)
    norms      6.0e-5, 1.0e-4, 4.8e-5, 5.4e-5, 6.5e-5, 2.3e-4 (4.4e-5)
    Adam       0.037,  0.242,  0.279,  0.149,  0.046,  0.075  (0.037)
    k_adam alone: 0 at every first step (the same bits); 0.96 at the second (one weight rounds the other way)
At B = 5 and 65 these are the figures of the CPU oracle against the restatement (tests/test_ballgame_reference.py): the
kernels accumulate in double and round to fp32 where they store, as the oracle does.

What this file found.  With fp32 accumulators (as the kernels were written) every edge was right, but B = 63 missed the Adam
tolerance: one weight of K1, var 2[493], ended 2.086e-7 from the restatement's (tolerance 2e-7; Q 4.1e-3, gradients 4.9e-4
of theirs).  Its gradient was -3.456e-8 on the GPU and -3.727e-8 in float64 - a sum of 567 products that nearly cancels,
2.7e-9 apart.  The first Adam step moves a weight by lr g / (|g| + eps / sqrt(1 - beta2)) = 2.5e-4 g / (|g| + 3.16e-6):
for |g| << 3e-6 its slope is 79, and 79 * 2.7e-9 = 2.1e-7.  The reductions of ballgame.hip now run in double (the same
element: -3.698e-8, |w - w_ref| 3.0e-8).
"""
import numpy as np
import pytest

import ballgame_reference as R
from test_gpu_ballgame import rand_obs

pytestmark = pytest.mark.gpu


def _qlx():
    import qlx
    return qlx


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def model_and_restatement(seed):
    qlx = _qlx()
    m = qlx.BallGameModel(seed=seed)
    w = R.nonzero_biases(m.weights())
    for v in (1, 3, 5, 7):
        m.set(v, w[v])
    return m, R.Net(w, qlx.model_hparams(ballgame=True))


def check_step(m, net, x, steps, tag):
    """One forward and one train step of model m on x against the restatement `net` (both advance by one step)."""
    B = x.shape[0]
    q, a = m.q_values(x)
    q64 = net.q_values(x)
    rq = R.q_ratio(q, q64)
    assert np.array_equal(a, q.argmax(axis=1))   # first maximum of the returned Q
    d = R.decided_rows(q64)
    assert np.array_equal(a[d], q64.argmax(axis=1)[d])
    mx = m.batch_predict_max_future_reward(x)
    assert np.array_equal(bits(mx), bits(q.max(axis=1)))
    acts, y = R.actions_and_targets(q64)
    before = [[m.get(v, which) for v in range(8)] for which in range(3)]
    loss, g, nrm = m.train(x, acts, y, want_grads=True)
    l64, g64, n64 = net.train(x, acts, y)
    ratios = R.step_ratios(loss, g, nrm, m.weights(), l64, g64, n64, net.w, steps)
    ratios["k_adam"] = R.own_adam_ratio(g, nrm, before, m.weights(), net.hp, steps)
    worst = max(ratios, key=ratios.get)
    print(f"{tag}: Q error / tolerance {rq:.2e} ({int(d.sum())} of {B} rows decided); loss {ratios['loss']:.2e}, "
          f"gradients {max(ratios[f'grad{v}'] for v in range(8)):.2e}, norms {max(ratios[f'norm{v}'] for v in range(8)):.2e}, "
          f"adam {max(ratios[f'adam{v}'] for v in range(8)):.2e}, k_adam on its own gradients {ratios['k_adam']:.2e}; "
          f"worst {worst} {ratios[worst]:.2e}; "
          f"{R.worst_adam_element(g, m.weights(), g64, net.w)}")
    assert rq <= 1.0, f"{tag}: Q is {rq:.2f} x its tolerance"
    bad = {k: round(r, 3) for k, r in ratios.items() if not r <= 1.0}
    assert not bad, f"{tag}: error / tolerance {bad}"


@pytest.mark.parametrize("B", [1, 3, 5, 63, 65, 100])
def test_forward_and_train_step(B):
    m, net = model_and_restatement(5)
    check_step(m, net, rand_obs(B, 9), 1, f"B={B}")
    assert m.iterations() == 1


def test_forward_is_batch_invariant():
    m, _ = model_and_restatement(5)
    x = rand_obs(100, 9)
    q, a = m.q_values(x)
    mx = m.batch_predict_max_future_reward(x)
    perm = np.random.default_rng(1).permutation(100)
    assert perm[64:].min() < 64 <= perm[:64].max()   # rows change tiles
    qp, ap = m.q_values(x[perm])
    assert np.array_equal(bits(qp), bits(q[perm])) and np.array_equal(ap, a[perm])
    assert np.array_equal(bits(m.batch_predict_max_future_reward(x[perm])), bits(mx[perm]))
    for i in (0, 63, 64, 99):
        q1, a1 = m.q_values(x[i:i + 1])
        assert np.array_equal(bits(q1[0]), bits(q[i])) and a1[0] == a[i], i
        assert np.array_equal(bits(m.batch_predict_max_future_reward(x[i:i + 1])), bits(mx[i:i + 1])), i


def test_second_step_at_a_smaller_batch():
    m, net = model_and_restatement(5)
    check_step(m, net, rand_obs(100, 9), 1, "B=100")
    check_step(m, net, rand_obs(37, 10), 2, "then B=37")
    assert m.iterations() == 2
