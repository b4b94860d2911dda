"""bf16 Q-net at ragged batch sizes, element by element and block by block against the teacher-forced emulation
(tests/bf16_reference.py forward_backward_full with the product's own stored a1..a4 and Q; bounds: tests/bf16_checks.py,
which tests/test_bf16_reference_bounds.py holds the emulation itself to on the CPU).

Forward (B = 1, 37, 87, 129, 200, 257, 520), per element of every stored activation:
    |gpu - emu| <= ulp_bf16(max(|gpu|, |emu|)) + 2 K 2^-24 S        (K = 256, 512, 576, 3136; S = sum |a||w| + |b|)
  share of unequal elements per layer <= 10 x the CPU's float32-vs-float64 share (caps 1.6e-4, 1.6e-4, 3.5e-4, 5.3e-4)
  Q vs a4_gpu W4 + b4 in float64: <= 2 * 512 * 2^-24 * S per element; max-Q and argmax exactly those of the returned Q.
  Measured on the MI355X over the seven B: activation error / bound <= 0.955 (one rounding flip is the whole first term);
  shares of unequal elements at most a1 9.1e-6, a2 1.06e-4, a3 4.8e-5, a4 1.56e-4; Q error / bound <= 1e-3.
Training step (B = 1, 37, 87, 129, 200, 257):
  loss, dW4, db4 against float64 from the product's own Q, a4, actions, y: <= 2 B 2^-24 sum |terms| (derived)
  every other gradient block-wise (dW3 in its 25 x 4 tiles, conv kernels per tap, biases whole) against the forced emulation:
    largest block error measured on the MI355X, B = 1 .. 257: 1.0e-7, 6.35e-4, 1.15e-4, 5.4e-5, 1.72e-4, 1.57e-4 (all in dW0
    taps or b1; the float32 emulation on the CPU: 2.4e-4).  4 x the largest is 2.5e-3, above the 2e-3 ceiling that the
    whole-variable check of tests/test_gpu_qnet_bf16.py sets, so BLOCK_REL = 2e-3 (3.1 x the largest; the runs are
    deterministic).  What is left is not the head (restating it in float32 changed no figure) but bf16 rounding flips of
    the stored dz3 / dz2 / dz1, which the product does not expose and the emulation therefore cannot be forced with.
  norms[v] against sqrt(sum g^2) in float64 of the returned gradients: relative <= 1e-5 (a partial's longest fp32 add
  chain is ~100 adds; a lost dW3 tile moves the norm by ~5e-3).
"""
import ctypes
import functools

import numpy as np
import pytest

import bf16_checks as C
import bf16_reference
import oracle as O

pytestmark = pytest.mark.gpu

PER_SAMPLE = (12800, 5184, 3136, 512)
ACT_SHAPES = ((20, 20, 32), (9, 9, 64), (7, 7, 64), (512,))


def _qlx():
    import qlx
    return qlx


@functools.lru_cache(maxsize=None)
def _env_frames(n):
    """Real Breakout observations from the oracle env (random play)."""
    env, out, rng = O.Env(seed=123), [], np.random.default_rng(5)
    while len(out) < n:
        r, d = env.step(int(rng.integers(0, 3)))
        out.append(env.tensor())
        if d:
            env.reset()
    return np.stack(out)


def states(B, seed):
    """Half oracle-env frames, half dense random frames."""
    dense = np.random.default_rng(seed).integers(0, 256, size=(B - B // 2, 84, 84, 4), dtype=np.uint8)
    return np.concatenate([_env_frames(260)[:B // 2], dense]) if B > 1 else dense


def bf16_model(seed, bias_seed):
    """A bf16 model with non-zero biases, and its weights."""
    qlx = _qlx()
    m = qlx.DeepQLearningModel(seed=seed, precision=qlx.PREC_BF16)
    w = C.nonzero_biases(m.weights(), bias_seed)
    m.set_weights(w)
    return m, w


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def fresh_copy(live, path):
    """A new model with the live one's weights, Adam slots and iteration count (through a checkpoint, which carries all)."""
    qlx = _qlx()
    live.write_checkpoint(path)
    m = qlx.DeepQLearningModel(seed=1, precision=qlx.PREC_BF16)
    m.read_checkpoint(path)
    assert m.iterations() == live.iterations()
    for v in range(10):
        for which in range(3):
            assert np.array_equal(bits(m.get(v, which)), bits(live.get(v, which)))
    return m


def stored_activations(m, B):
    out = []
    for layer in range(1, 5):
        got = np.zeros(PER_SAMPLE[layer - 1] * B, np.float32)
        assert _qlx().lib().qlx_model_last_activation(m.h, layer, got.ctypes.data_as(ctypes.c_void_p)) == 0
        out.append(got.reshape((B,) + ACT_SHAPES[layer - 1]))
    return out


def check_forward(m, w, x, tag):
    """Item 2 of the module docstring for one forward of model m (weights w) on x; returns (q, actions, activations)."""
    B = x.shape[0]
    q, a = m.q_values(x)
    acts = stored_activations(m, B)
    emu = bf16_reference.forward_backward_full(w, x, acts=acts)
    for l in range(4):
        ratio, share, i = C.activation_check(acts[l], emu["acts"][l], emu["S"][l], C.LAYER_K[l])
        print(f"{tag} a{l + 1}: error / bound {ratio:.3f}, unequal share {share:.2e} (cap {C.SHARE_CAP[l]:.1e})")
        assert ratio <= 1.0, f"{tag} a{l + 1}: element {i} (sample {i // PER_SAMPLE[l]}) is {ratio:.2f} x its bound"
        assert share <= C.SHARE_CAP[l], f"{tag} a{l + 1}: {share:.2e} of the elements differ"
    w4, b4 = w[8].astype(np.float64), w[9].astype(np.float64)
    a4 = acts[3].astype(np.float64)
    q_ref, q_bound = a4 @ w4 + b4, 2 * 512 * C.U24 * (np.abs(a4) @ np.abs(w4) + np.abs(b4))
    print(f"{tag} Q: error / bound {(np.abs(q - q_ref) / q_bound).max():.3f}, max|Q| {np.abs(q).max():.1f}")
    assert (np.abs(q - q_ref) <= q_bound).all()
    assert np.array_equal(a, np.argmax(q, axis=1))
    mx = m.batch_predict_max_future_reward(x)
    assert np.array_equal(mx.view(np.uint32), q.max(axis=1).view(np.uint32))
    return q, a, acts


@pytest.mark.parametrize("B", [1, 37, 87, 129, 200, 257, 520])
def test_forward_elementwise(B):
    m, w = bf16_model(7, 100 + B)
    check_forward(m, w, states(B, B), f"B={B}")


# Each B with the paths it is the smallest (or only) shape to reach:
#   1    fc1 wgrad nk = 1 with 31 zero k-rows; a single block everywhere; three idle head waves
#   37   nk = 2 (the short prologue) with ragged K; conv wgrad `used` = 37 padded to 40 blocks; B % 4 = 1
#   87   nk = 3; conv3 per3 = 2 with a one-sample last chunk (used3 = 44 -> 48)
#   129  nk = 5 (remainder step 1), the last k-step holds one row; conv2 per2 = 2, used2 = 65 -> 72, last chunk one sample;
#        the second fc1 backward-data M tile holds one row
#   200  nk = 7 (remainder 3), ragged K
#   257  nk = 9; block 0 of every trunk kernel owns two samples, the others one
@pytest.mark.parametrize("B", [1, 37, 87, 129, 200, 257])
def test_train_step_blockwise(B):
    m, w = bf16_model(7, 100 + B)
    x = states(B, B)
    q, _ = m.q_values(x)
    acts = stored_activations(m, B)
    rng = np.random.default_rng(B)
    a = rng.integers(0, 3, B).astype(np.uint8)
    y = (q[np.arange(B), a] + rng.normal(0, 1.5, B)).astype(np.float32)
    e = np.abs(q[np.arange(B), a] - y)
    assert B == 1 or ((e < 1).any() and (e > 1).any())   # both Huber branches
    loss, grads, norms = m.train(x, a, y, want_grads=True)
    for l, again in enumerate(stored_activations(m, B)):   # the training forward stored what the plain forward stored
        assert np.array_equal(again, acts[l]), f"a{l + 1} of the training forward"
    # derived: the head from the product's own Q and a4
    head = C.head_reference(q, acts[3], a, y)
    print(f"B={B} loss error / bound {abs(loss - head['loss'][0]) / head['loss'][1]:.3f}")
    assert abs(loss - head["loss"][0]) <= head["loss"][1], (loss, head["loss"])
    for v, key in ((8, "dW4"), (9, "db4")):
        ref, bound = head[key]
        bad = np.argwhere(np.abs(grads[v] - ref) > bound)
        print(f"B={B} {key} error / bound {(np.abs(grads[v] - ref) / np.maximum(bound, 1e-300)).max():.3f}")
        assert bad.size == 0, f"{key}: {len(bad)} elements past their bound, first {bad[0]}"
    # block-wise against the forced emulation
    emu = bf16_reference.forward_backward_full(w, x, a, y, acts=acts, q=q)
    worst = ("", 0.0)
    failures = []
    for v in range(10):
        for label, err in C.block_errors(grads[v], emu["grads"][v], v):
            worst = max(worst, (f"var{v} {label}", err), key=lambda t: t[1])
            if err > C.BLOCK_REL:
                failures.append(f"var{v} {label}: {err:.2e}")
    print(f"B={B} largest gradient block error {worst[1]:.2e} ({worst[0]})")
    assert not failures, f"{len(failures)} blocks past {C.BLOCK_REL:.1e}: " + "; ".join(failures[:8])
    # the norms are those of the gradients the same call returned
    for v in range(10):
        want = np.sqrt((grads[v].astype(np.float64) ** 2).sum())
        assert abs(norms[v] - want) <= 1e-5 * want, f"norm of var {v}: {norms[v]} vs {want}"
