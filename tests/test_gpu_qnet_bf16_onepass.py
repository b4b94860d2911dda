"""The bf16 one-pass fc1 (qnet_bf16.hip bf16_forward: CfgFc1FwdBig + Epi4BiasRelu, 128 x 128 tiles, bias + ReLU + bf16 in the
epilogue) element by element at ragged batches, the batch invariance the target memo rests on, and the learner's bf16
Bellman targets composed from the forward pinned here.

Which models take the one-pass path: every bf16 learner's target net at every batch size - learner.hip's
qlx_learner_create calls model_set_batch_invariant(L->target), which sets fc1_single - and any bf16 model at B >= 8192.  The
target net is reached without new ABI: SelfDrivingQLearner(...).stabilized_model is a DeepQLearningModel over it.  The
elementwise tests of tests/test_gpu_qnet_bf16_shapes.py build plain models only, so they reach the split-K path only
(CfgFc1Fwd + Epi4Slab, four fp32 slabs the head sums).

A1  check_forward of tests/test_gpu_qnet_bf16_shapes.py (bounds: tests/bf16_checks.py, unchanged) on the target net at
    B = 1, 37, 129, 257: 1, 1, 2, 3 M tiles whose last holds 1, 37, 1, 1 rows; tiles() = 4, 4, 8, 12 on an xcd_grid of
    8, 8, 8, 16 (idle blocks and the XCD tile remap both in play).
A2  300 samples; Q and the stored a1..a4 rows of a sample are the same bits alone at B = 1, in a batch of 37, at B = 300
    (samples 256.. are the second sample of a persistent trunk block, trunk_grid = 256, and sit in the third M tile) and
    after a fixed permutation of the 300.  On the target net and on a plain model (split-K below 8192: four slabs
    summed in order, each slab's k order fixed by the tile, so bit-invariant as well; this is also the "conv trunk is
    per sample" claim of tests/test_gpu_qnet_bf16.py, and it catches LDS state carried between a block's samples).
A3  a plain model at B = 8192 + 37 (65 M tiles, 260 tiles on a grid of 264, last tile 37 rows), dense random frames: fc1
    teacher-forced from the product's own a3 in float64 over every row, Q from its own a4, and the first 64 rows' Q
    bit-equal to the target net of A1 on the same frames (the same kernel).
A4  a bf16 learner (64 envs, B = 37, 8 updates per vector step: the per-batch target pass runs 296 rows = 3 M tiles, the
    last of 40 rows; the memo fills run 64 rows), with and without the target memo, and with double DQN:
    targets[u] == where(done, r, fl32(r + fl32(max_a Q_target(s') gamma))) bit for bit, Q_target from
    L.stabilized_model.q_values on the sampled transitions (a* from a copy of the online net for double DQN).

Measured on the MI355X.  A1, over the four B: activation error / bound <= 0.955 (one rounding flip is the whole first term);
shares of unequal elements at most a1 9.1e-6, a2 1.7e-5, a3 3.1e-5, a4 1.06e-4 - the one 3136-long fp32 chain of the
one-pass kernel stays under the a4 cap of the split path (5.3e-4; the split path itself measures 1.56e-4), so
tests/bf16_checks.py is used as it stands; Q error / bound <= 1e-3.  A3: a4 error / bound 0.541, share 8.2e-5, Q error /
bound 1e-3; its two float64 GEMMs take 1.3 s on 16 threads, so every row is checked.  A4: 17 vector steps checked per run
(170 played); the checked batches held one transition with done and 31 with a reward and no done.

What A4 found: k_fc2<2> formed r + max_a Q gamma as one fused multiply-add (qnet_bf16.hip is built with contraction on and
__fadd_rn / __fmul_rn are plain operators in a header), one rounding where the reference and the fp32 path round twice.
The memo and the per-batch pass shared the kernel, so they agreed with each other; the head now rounds twice.
With r = 0 both forms give the same bits, so the test asserts that it checked rewarded transitions too.
"""
import ctypes

import numpy as np
import pytest

import bf16_checks as C
import bf16_reference
from test_gpu_qnet_bf16_shapes import PER_SAMPLE, bf16_model, bits, check_forward, fresh_copy, states, stored_activations

pytestmark = pytest.mark.gpu


def _qlx():
    import qlx
    return qlx


def target_net(bias_seed, seed=7):
    """(learner, its target net - batch invariant, so fc1 in one pass at every B - with non-zero biases, the weights)."""
    qlx = _qlx()
    L = qlx.SelfDrivingQLearner(qlx.Parameter(n_envs=8, batch_size=8, history_buffer_len=64, init_seed=seed,
                                              stats_after_steps=0, qnet_precision=qlx.PREC_BF16))
    w = C.nonzero_biases(L.stabilized_model.weights(), bias_seed)
    L.stabilized_model.set_weights(w)
    return L, L.stabilized_model, w


@pytest.mark.parametrize("B", [1, 37, 129, 257])
def test_one_pass_forward_elementwise(B):
    L, m, w = target_net(100 + B)
    check_forward(m, w, states(B, B), f"one-pass B={B}")
    L.close()


SAMPLES = (0, 36, 127, 128, 255, 256, 299)


def forward_bits(m, x):
    q, a = m.q_values(x)
    return [bits(q), a] + [bits(act) for act in stored_activations(m, x.shape[0])]


def check_invariance(m, tag):
    x = states(300, 3)
    names = ("Q", "argmax", "a1", "a2", "a3", "a4")
    base = forward_bits(m, x)

    def same(got, rows, what):
        for name, g, b in zip(names, got, base):
            assert np.array_equal(g, b[rows]), f"{tag} {name}: {what}"

    for s in SAMPLES:   # alone
        same(forward_bits(m, x[s:s + 1]), [s], f"sample {s} alone at B = 1 against its row at B = 300")
    rng = np.random.default_rng(11)
    others = np.setdiff1d(np.arange(300), SAMPLES)
    idx = rng.permutation(np.concatenate([SAMPLES, rng.choice(others, 37 - len(SAMPLES), replace=False)]))
    same(forward_bits(m, x[idx]), idx, "a batch of 37 against its rows at B = 300")
    perm = rng.permutation(300)
    assert (perm[256:] < 128).any() and (perm[:128] >= 256).any()   # rows change M tiles and trunk blocks
    same(forward_bits(m, x[perm]), perm, "q(x[perm]) against q(x)[perm]")


def test_target_net_is_batch_invariant():
    L, m, _ = target_net(3)
    check_invariance(m, "one-pass")
    L.close()


def test_plain_model_is_batch_invariant_below_8192():
    m, _ = bf16_model(7, 3)
    check_invariance(m, "split-K")


def test_one_pass_forward_at_8229():
    B = 8192 + 37
    m, w = bf16_model(7, 5)
    x = np.random.default_rng(B).integers(0, 256, size=(B, 84, 84, 4), dtype=np.uint8)
    q, a = m.q_values(x)
    acts = []
    for layer in (3, 4):
        got = np.zeros(PER_SAMPLE[layer - 1] * B, np.float32)
        assert _qlx().lib().qlx_model_last_activation(m.h, layer, got.ctypes.data_as(ctypes.c_void_p)) == 0
        acts.append(got.reshape(B, -1).astype(np.float64))
    a3, a4 = acts
    import torch
    w3 = bf16_reference.bf16(torch.as_tensor(np.asarray(w[6], np.float64))).numpy()
    b3 = np.asarray(w[7], np.float64)
    ref = bf16_reference.bf16(torch.as_tensor(np.maximum(a3 @ w3 + b3, 0.0))).numpy()
    S = np.abs(a3) @ np.abs(w3) + np.abs(b3)
    ratio, share, i = C.activation_check(a4, ref, S, 3136)
    print(f"B={B} a4: error / bound {ratio:.3f}, unequal share {share:.2e} (cap {C.SHARE_CAP[3]:.1e})")
    assert ratio <= 1.0, f"a4 element {i} (sample {i // 512}) is {ratio:.2f} x its bound"
    assert share <= C.SHARE_CAP[3], f"a4: {share:.2e} of the elements differ"
    w4, b4 = w[8].astype(np.float64), w[9].astype(np.float64)
    q_ref, q_bound = a4 @ w4 + b4, 2 * 512 * C.U24 * (np.abs(a4) @ np.abs(w4) + np.abs(b4))
    print(f"B={B} Q: error / bound {(np.abs(q - q_ref) / q_bound).max():.3f}, max|Q| {np.abs(q).max():.1f}")
    assert (np.abs(q - q_ref) <= q_bound).all()
    assert np.array_equal(a, np.argmax(q, axis=1))
    mx = m.batch_predict_max_future_reward(x)
    assert np.array_equal(bits(mx), bits(q.max(axis=1)))
    # the same kernel as the target net's: the same bits
    L, t, _ = target_net(5)
    t.set_weights(w)
    q64, a64 = t.q_values(x[:64])
    assert np.array_equal(bits(q64), bits(q[:64])) and np.array_equal(a64, a[:64])
    L.close()


def bellman(q, q_select, batch, gamma):
    v = q.max(axis=1) if q_select is None else q[np.arange(q.shape[0]), np.argmax(q_select, axis=1)]
    y = batch["reward"] + v * np.float32(gamma)   # two float32 roundings
    assert v.dtype == y.dtype == np.float32
    return np.where(batch["done"], batch["reward"], y)


def target_learner(flags=0):
    qlx = _qlx()
    L = qlx.SelfDrivingQLearner(qlx.Parameter(n_envs=64, batch_size=37, update_after_actions=8, history_buffer_len=20_000,
                                              target_sync_steps=0, epsilon_pure_random_steps=10**9, stats_after_steps=0,
                                              flags=flags, qnet_precision=qlx.PREC_BF16))
    L.stabilized_model.set_weights(C.nonzero_biases(L.stabilized_model.weights(), 9))   # (the memo is rebuilt on a write)
    return L


@pytest.mark.parametrize("cache", [1, 0])
def test_learner_targets_are_the_pinned_forward(monkeypatch, cache):
    monkeypatch.setenv("QLX_TARGET_CACHE", str(cache))
    L = target_learner()
    gamma = L.param.gamma
    steps_checked = dones_checked = rewarded_checked = 0
    for step in range(400):
        L.vector_step()
        g = L.last()
        assert g["targets"].shape == (8, 37)
        batches = [L.replay_buffer.get_many(g["indices"][u]) for u in range(8)]
        n_done = sum(int(b["done"].sum()) for b in batches)
        if step % 10 and not n_done:
            continue
        for u, batch in enumerate(batches):
            q = L.stabilized_model.q_values(batch["state_next"])[0]
            assert np.array_equal(bits(g["targets"][u]), bits(bellman(q, None, batch, gamma))), (step, u)
        steps_checked += 1
        dones_checked += n_done
        rewarded_checked += sum(int(((b["reward"] != 0) & ~b["done"]).sum()) for b in batches)
        if dones_checked and rewarded_checked and steps_checked >= 12:
            break
    print(f"cache={cache}: {steps_checked} vector steps checked, {dones_checked} sampled transitions with done, "
          f"{rewarded_checked} with a reward and no done")
    assert dones_checked > 0
    assert rewarded_checked > 0   # with r = 0 the sum r + v gamma rounds once however it is formed
    L.close()


def test_double_dqn_learner_targets_are_the_pinned_forward(tmp_path):
    """a* = first argmax of the online net as it stands before the step's updates (split-K path at 296 rows, invariant by
    test_plain_model_is_batch_invariant_below_8192), the value from the target net."""
    qlx = _qlx()
    L = target_learner(flags=qlx.DOUBLE_DQN)
    gamma = L.param.gamma
    other = 0
    for step in range(41):
        sel = fresh_copy(L.model, str(tmp_path / "online.ckpt")) if step % 10 == 0 else None
        L.vector_step()
        if sel is None:
            continue
        g = L.last()
        for u in range(8):
            batch = L.replay_buffer.get_many(g["indices"][u])
            q = L.stabilized_model.q_values(batch["state_next"])[0]
            qs = sel.q_values(batch["state_next"])[0]
            other += int((np.argmax(qs, axis=1) != np.argmax(q, axis=1)).sum())
            assert np.array_equal(bits(g["targets"][u]), bits(bellman(q, qs, batch, gamma))), (step, u)
    print(f"double DQN: {other} sampled transitions whose a* is not the target net's own argmax")
    assert other > 0
    L.close()
