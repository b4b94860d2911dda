"""Bounds and block cuts shared by the bf16 Q-net shape tests (GPU: tests/test_gpu_qnet_bf16_shapes.py, tests/
test_gpu_qnet_bf16_update.py) and the CPU test that holds the emulation itself to them (tests/test_bf16_reference_bounds.py).

Forward, per element of a stored activation (layer reduction length K, S = sum |a||w| + |b| of that element):
    |got - emu| <= ulp_bf16(max(|got|, |emu|)) + 2 K 2^-24 S
one bf16 rounding flip plus the worst-case error of an fp32 sum of K products; both derived, nothing tuned.

Share of unequal elements per layer: measured for float32 against float64 accumulation on the CPU (both forced with the float64
activations, B = 5 and 37, tests/test_bf16_reference_bounds.py prints them):
    a1 1.6e-5, a2 1.6e-5, a3 3.4e-5, a4 5.3e-5 at the most
The cap is 10 x that (an MFMA reduction's order is not the CPU's), and never above 1 % of the layer.

Gradients, block-wise: relative L2 per block, blocks cut along the kernels' seams (gradient_blocks), denominator the
block's reference norm + 1e-3 rms(variable) sqrt(block size).  BLOCK_REL: the largest block error measured on the MI355X
over B = 1, 37, 87, 129, 200, 257 is 6.35e-4 (tests/test_gpu_qnet_bf16_shapes.py states every figure); 4 x that (2.5e-3) is
above the 2e-3 ceiling that the whole-variable bound of tests/test_gpu_qnet_bf16.py sets, so the ceiling is the threshold.
"""
import numpy as np

U24 = 2.0 ** -24
LAYER_K = (256, 512, 576, 3136)
SHARE_MEASURED = (1.6e-5, 1.6e-5, 3.5e-5, 5.3e-5)
SHARE_CAP = tuple(min(10.0 * s, 1e-2) for s in SHARE_MEASURED)
BLOCK_REL = 2e-3


def ulp_bf16(x):
    """Spacing of bf16 (8 significant bits) at |x|; 0 at 0."""
    x = np.abs(np.asarray(x, np.float64))
    _, e = np.frexp(x)   # x = m 2^e, m in [0.5, 1)
    return np.where(x > 0, np.ldexp(1.0, e - 8), 0.0)


def activation_check(got, emu, S, K):
    """(worst |got - emu| / bound, share of unequal elements, index of the worst) of one layer."""
    got, emu, S = (np.asarray(a, np.float64).ravel() for a in (got, emu, S))
    d = np.abs(got - emu)
    bound = ulp_bf16(np.maximum(np.abs(got), np.abs(emu))) + 2.0 * K * U24 * S
    ratio = np.where(d > 0, d / np.maximum(bound, 1e-300), 0.0)
    i = int(np.argmax(ratio))
    return float(ratio[i]), float((d > 0).mean()), i


def gradient_blocks(v):
    """(label, index) pairs cutting variable v's gradient (Keras layout) along the kernels' seams."""
    if v in (0, 2, 4):   # conv kernels [kh][kw][c][oc]: one block per tap
        n = (8, 4, 3)[v // 2]
        return [(f"tap({kh},{kw})", (kh, kw)) for kh in range(n) for kw in range(n)]
    if v == 6:   # full_layer kernel [3136][512]: the weight gradient's 25 x 4 tiles of 128 x 128 (the last holds 64 rows)
        return [(f"tile({i},{j})", (slice(128 * i, min(3136, 128 * i + 128)), slice(128 * j, 128 * j + 128)))
                for i in range(25) for j in range(4)]
    return [("all", Ellipsis)]


def block_errors(g, ge, v):
    """[(label, relative L2 error)] of gradient g against the reference ge over variable v's blocks."""
    g, ge = np.asarray(g, np.float64), np.asarray(ge, np.float64)
    rms = np.sqrt(np.mean(ge ** 2))
    out = []
    for label, idx in gradient_blocks(v):
        a, b = g[idx], ge[idx]
        out.append((label, float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-3 * rms * np.sqrt(b.size) + 1e-300))))
    return out


def head_reference(q, a4, actions, y):
    """Loss, dW4, db4 in float64 from the product's own Q, a4, actions and y, each with its bound 2 B 2^-24 sum |terms|."""
    q, a4, y = np.asarray(q, np.float64), np.asarray(a4, np.float64), np.asarray(y, np.float64)
    B = q.shape[0]
    e = q[np.arange(B), actions] - y
    h = np.where(np.abs(e) <= 1.0, 0.5 * e * e, np.abs(e) - 0.5)
    g = np.clip(e, -1.0, 1.0) / B
    onehot = np.zeros((B, 3))
    onehot[np.arange(B), actions] = 1.0
    gq = g[:, None] * onehot                       # dloss / dq [B][3]
    f = 2.0 * B * U24
    return dict(loss=(h.sum() / B, f * h.sum() / B), dW4=(a4.T @ gq, f * (np.abs(a4).T @ np.abs(gq))),
                db4=(gq.sum(0), f * np.abs(gq).sum(0)))


def nonzero_biases(weights, seed):
    """The given weights with the (initially zero) biases drawn from N(0, 0.05)."""
    rng = np.random.default_rng(seed)
    return [rng.normal(0, 0.05, w.shape).astype(np.float32) if v % 2 else np.asarray(w, np.float32) for v, w in enumerate(weights)]


def adam_alpha(hp, t):
    """model_adam's alpha = lr sqrt(1 - beta2^t) / (1 - beta1^t) in float32 (powers rounded once to float32)."""
    lr, b1, b2 = np.float32(hp[0]), np.float32(hp[1]), np.float32(hp[2])
    b1p, b2p = np.float32(np.float64(b1) ** t), np.float32(np.float64(b2) ** t)
    one = np.float32(1.0)
    return np.float32(np.float32(lr * np.sqrt(one - b2p)) / np.float32(one - b1p))


def adam_step(g, norm, w, m, v, hp, t, scale=1.0):
    """adam_elem (q-learning_amd/csrc/qnet_bf16.hip) in numpy float32, one rounded operation per line."""
    f = np.float32
    lr, beta1, beta2, eps, clipnorm = (f(x) for x in hp)
    g, w, m, v = (np.asarray(a, f) for a in (g, w, m, v))
    alpha = adam_alpha(hp, t)
    denom = np.maximum(f(norm), clipnorm)
    gs = g * f(scale)
    gs = gs * clipnorm
    gc = gs / denom
    d = gc - m
    d = d * f(f(1.0) - beta1)
    m = m + d
    s = gc * gc
    s = s - v
    s = s * f(f(1.0) - beta2)
    v = v + s
    r = np.sqrt(v)
    r = r + eps
    n = m * alpha
    n = n / r
    w = w - n
    assert w.dtype == m.dtype == v.dtype == np.float32
    return w, m, v
