"""The bf16 emulation (tests/bf16_reference.py) held to the bounds the GPU kernels are held to (tests/bf16_checks.py):
the same contract in float32 accumulation against float64 accumulation, both teacher-forced with the float64 run's
stored activations.  The reference alone stays inside every bound, so a GPU failure is the kernel's.

Measured here (B = 5 / 37): activation error / bound <= 0.91; shares of unequal elements a1 1.6e-5 / 8.4e-6, a2 0 / 1.6e-5,
a3 0 / 3.4e-5, a4 0 / 5.3e-5 (the caps in tests/bf16_checks.py are 10 x the larger); Q error / bound <= 1e-3; largest
gradient block error 2.4e-4 / 1.8e-4 (BLOCK_REL = 2e-3).  Both runs take about 4 s together.
"""
import numpy as np
import pytest
import torch

import bf16_checks as C
import bf16_reference
import oracle as O


def states(B, seed):
    """Half oracle-env frames (random play), half dense random frames."""
    env, out, rng = O.Env(seed=123), [], np.random.default_rng(5)
    while len(out) < B // 2:
        r, d = env.step(int(rng.integers(0, 3)))
        out.append(env.tensor())
        if d:
            env.reset()
    dense = np.random.default_rng(seed).integers(0, 256, size=(B - B // 2, 84, 84, 4), dtype=np.uint8)
    return np.concatenate([np.stack(out), dense]) if out else dense


@pytest.mark.parametrize("B", [5, 37])
def test_float32_emulation_inside_the_gpu_bounds(B):
    w = C.nonzero_biases(O.QNet(seed=7).weights(), 100 + B)
    x = states(B, B)
    rng = np.random.default_rng(B)
    a = rng.integers(0, 3, B).astype(np.uint8)
    free = bf16_reference.forward_backward_full(w, x)
    q = free["q"].astype(np.float32)   # the Q the loss is taken at: a float32 array, as the product's is
    y = (q[np.arange(B), a] + rng.normal(0, 1.5, B)).astype(np.float32)
    acts = free["acts"]
    r64 = bf16_reference.forward_backward_full(w, x, a, y, acts=acts, q=q)
    r32 = bf16_reference.forward_backward_full(w, x, a, y, acts=acts, q=q, dtype=torch.float32)
    for l in range(4):   # forcing a float64 run with its own activations changes nothing
        assert np.array_equal(r64["acts"][l], acts[l])
    for l in range(4):
        ratio, share, i = C.activation_check(r32["acts"][l], r64["acts"][l], r64["S"][l], C.LAYER_K[l])
        print(f"B={B} a{l + 1}: error / bound {ratio:.3f}, unequal share {share:.2e} (cap {C.SHARE_CAP[l]:.1e})")
        assert ratio <= 1.0, f"a{l + 1} element {i}"
        assert share <= C.SHARE_CAP[l], f"a{l + 1}"
    w4, b4 = w[8].astype(np.float64), w[9].astype(np.float64)
    q_ref = acts[3] @ w4 + b4
    q_bound = 2 * 512 * C.U24 * (np.abs(acts[3]) @ np.abs(w4) + np.abs(b4))
    print(f"B={B} Q: error / bound {(np.abs(r32['q'] - q_ref) / q_bound).max():.3f}")
    assert (np.abs(r32["q"] - q_ref) <= q_bound).all()
    head = C.head_reference(q, acts[3], a, y)   # the Q that the loss was taken at
    assert abs(r32["loss"] - head["loss"][0]) <= head["loss"][1]
    assert (np.abs(r32["grads"][8] - head["dW4"][0]) <= head["dW4"][1]).all()
    assert (np.abs(r32["grads"][9] - head["db4"][0]) <= head["db4"][1]).all()
    worst = ("", 0.0)
    for v in range(10):
        for label, err in C.block_errors(r32["grads"][v], r64["grads"][v], v):
            worst = max(worst, (f"var{v} {label}", err), key=lambda t: t[1])
            assert err <= C.BLOCK_REL, f"var {v} {label}: {err:.2e}"
    print(f"B={B} largest gradient block error {worst[1]:.2e} ({worst[0]})")
