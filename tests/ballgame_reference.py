"""Float64 numpy restatement of the BallGame Q-model (test infrastructure), written from the model description in
q-learning_amd/csrc/ballgame.hip's header comment and from oracle/ballgame_ref.cpp:

    x [B][3][3][4] u8 one-hot
    Conv2D 32 2x2 'same' (TF pads a 2x2 kernel with one zero row / column *after* the data), ReLU   -> a1 [B][3][3][32]
    Conv2D 32 1x1, ReLU                                                                             -> a2 [B][3][3][32]
    Flatten (i, j, c), Dense 512, ReLU                                                              -> a3 [B][512]
    Dense 5                                                                                         -> q  [B][5]
    loss = mean_b (q[b][a_b] - y_b)^2;  dloss/dq[b][a_b] = 2 e_b / B

Everything up to and including the gradients and their per-variable L2 norms is float64 matrix algebra in the Keras
layouts (kernels [kh][kw][c][oc] / [in][out]); nothing follows a kernel's reduction order.  The optimizer step (legacy Keras
Adam with clip_by_norm per variable) is restated from k_adam in float32 with one rounding per operation, as
bf16_checks.adam_step does for the Breakout net: it is applied to the float64 gradients rounded once to float32.
"""
import numpy as np

VAR_SHAPES = [(2, 2, 4, 32), (32,), (1, 1, 32, 32), (32,), (288, 512), (512,), (512, 5), (5,)]
VAR_SIZES = [int(np.prod(s)) for s in VAR_SHAPES]


def _padded(x):
    """x [B][3][3][4] with TF's trailing zero row and column of a 2x2 'same' convolution."""
    x = np.asarray(x, np.float64)
    xp = np.zeros((x.shape[0], 4, 4, 4))
    xp[:, :3, :3] = x
    return xp


def forward(weights, x):
    """dict(q, a1, a2, a3) in float64 for weights (8 arrays, Keras layouts) and observations x [B][3][3][4]."""
    k0, b0, k1, b1, w2, b2, w3, b3 = (np.asarray(w, np.float64).reshape(s) for w, s in zip(weights, VAR_SHAPES))
    xp = _padded(x)
    B = xp.shape[0]
    z1 = b0 + sum(xp[:, di:di + 3, dj:dj + 3] @ k0[di, dj] for di in range(2) for dj in range(2))
    a1 = np.maximum(z1, 0.0)
    a2 = np.maximum(a1 @ k1[0, 0] + b1, 0.0)
    a3 = np.maximum(a2.reshape(B, 288) @ w2 + b2, 0.0)
    return dict(q=a3 @ w3 + b3, a1=a1, a2=a2, a3=a3)


def loss_and_gradients(weights, x, actions, y):
    """(q, loss, [8 gradients in the Keras layouts], norms[8]) in float64."""
    k1, w2, w3 = (np.asarray(weights[v], np.float64).reshape(VAR_SHAPES[v]) for v in (2, 4, 6))
    f = forward(weights, x)
    q, a1, a2, a3 = f["q"], f["a1"], f["a2"], f["a3"]
    xp = _padded(x)
    B, ar = q.shape[0], np.arange(q.shape[0])
    act = np.asarray(actions, np.int64)
    e = q[ar, act] - np.asarray(y, np.float64)
    dq = np.zeros((B, 5))
    dq[ar, act] = 2.0 * e / B
    a2f = a2.reshape(B, 288)
    dz3 = (dq @ w3.T) * (a3 > 0)
    dz2 = ((dz3 @ w2.T) * (a2f > 0)).reshape(B, 3, 3, 32)
    dz1 = (dz2 @ k1[0, 0].T) * (a1 > 0)
    g0 = np.zeros(VAR_SHAPES[0])
    for di in range(2):
        for dj in range(2):
            g0[di, dj] = np.einsum("bijc,bijo->co", xp[:, di:di + 3, dj:dj + 3], dz1)
    grads = [g0, dz1.sum((0, 1, 2)), np.einsum("bijc,bijo->co", a1, dz2).reshape(VAR_SHAPES[2]), dz2.sum((0, 1, 2)),
             a2f.T @ dz3, dz3.sum(0), a3.T @ dq, dq.sum(0)]
    norms = np.array([np.sqrt((g ** 2).sum()) for g in grads])
    return q, float((e ** 2).mean()), grads, norms


def adam_alpha(hp, t):
    """apply_adam's alpha = lr sqrt(1 - beta2^t) / (1 - beta1^t) in float32 (powers rounded once to float32)."""
    f = np.float32
    lr, beta1, beta2 = f(hp[0]), f(hp[1]), f(hp[2])
    b1p, b2p = f(np.float64(beta1) ** t), f(np.float64(beta2) ** t)
    return f(f(lr * np.sqrt(f(f(1.0) - b2p))) / f(f(1.0) - b1p))


def adam_step(g, norm, w, m, v, hp, t):
    """k_adam (q-learning_amd/csrc/ballgame.hip) for one variable in numpy float32, one rounded operation per line."""
    f = np.float32
    lr, beta1, beta2, eps, clipnorm = (f(x) for x in hp)
    g, w, m, v = (np.asarray(a, f) for a in (g, w, m, v))
    alpha = adam_alpha(hp, t)
    gc = g * clipnorm
    gc = gc / np.maximum(f(norm), clipnorm)
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


class Net:
    """Weights (float32, as the product stores them), Adam slots and the iteration count, carried through train steps."""

    def __init__(self, weights, hp):
        self.w = [np.asarray(w, np.float32).reshape(s).copy() for w, s in zip(weights, VAR_SHAPES)]
        self.m = [np.zeros(s, np.float32) for s in VAR_SHAPES]
        self.v = [np.zeros(s, np.float32) for s in VAR_SHAPES]
        self.hp = np.asarray(hp, np.float32)
        self.iterations = 0

    def q_values(self, x):
        return forward(self.w, x)["q"]

    def train(self, x, actions, y):
        """One MSE step; (loss, gradients, norms) of the weights before the step, in float64."""
        _, loss, grads, norms = loss_and_gradients(self.w, x, actions, y)
        t = self.iterations + 1
        for i in range(8):
            self.w[i], self.m[i], self.v[i] = adam_step(grads[i].astype(np.float32), np.float32(norms[i]), self.w[i],
                                                        self.m[i], self.v[i], self.hp, t)
        self.iterations = t
        return loss, grads, norms


def nonzero_biases(weights):
    """The given weights with the (initially zero) biases set as tests/test_gpu_ballgame.py sets them."""
    return [np.linspace(-0.05, 0.05, w.size, dtype=np.float32) if v % 2 else np.asarray(w, np.float32)
            for v, w in enumerate(weights)]


def actions_and_targets(q_ref):
    """actions arange(B) % 5 and y = q_ref[a] + sin(arange(B)), the batch of tests/test_gpu_ballgame.py.  At B = 1 that y
    is q_ref[a] itself: the error, the loss and every gradient would be rounding noise of Q (~1e-8) and no relative
    tolerance means anything, so the single sample gets sin(1)."""
    B = q_ref.shape[0]
    a = (np.arange(B) % 5).astype(np.uint8)
    s = np.sin(np.arange(B) + (1 if B == 1 else 0))
    return a, (np.asarray(q_ref, np.float32)[np.arange(B), a] + s.astype(np.float32)).astype(np.float32)


# The tolerances of tests/test_gpu_ballgame.py (its docstring justifies them), as error / tolerance ratios: a check
# passes when its ratio is <= 1.

def q_ratio(q, q_ref):
    """Q against float64: rtol 1e-4, atol 1e-5 max(1, max |q_ref|)."""
    q, q_ref = np.asarray(q, np.float64), np.asarray(q_ref, np.float64)
    tol = 1e-5 * max(1.0, np.abs(q_ref).max()) + 1e-4 * np.abs(q_ref)
    return float((np.abs(q - q_ref) / tol).max())


def decided_rows(q_ref):
    """Rows whose top-2 margin in the reference exceeds what q_ratio <= 1 lets two entries move towards each other."""
    q_ref = np.asarray(q_ref, np.float64)
    top = np.sort(q_ref, axis=1)
    tol = 1e-5 * max(1.0, np.abs(q_ref).max()) + 1e-4 * np.abs(q_ref).max(axis=1)
    return top[:, -1] - top[:, -2] > 2.0 * tol


def step_ratios(loss, flat_grads, norms, weights, ref_loss, ref_grads, ref_norms, ref_weights, steps=1):
    """{check: error / tolerance} of one train step: loss 1e-4 relative, every variable's gradient 1e-3 relative L2, every
    norm 1e-3 relative, weights after `steps` Adam steps 2e-7 * steps absolute."""
    out = dict(loss=abs(loss - ref_loss) / (1e-4 * abs(ref_loss)))
    off = 0
    for v, n in enumerate(VAR_SIZES):
        g, r = np.asarray(flat_grads[off:off + n], np.float64), np.asarray(ref_grads[v], np.float64).ravel()
        out[f"grad{v}"] = float(np.linalg.norm(g - r) / (1e-3 * np.linalg.norm(r)))
        out[f"norm{v}"] = float(abs(norms[v] - ref_norms[v]) / (1e-3 * ref_norms[v]))
        d = np.abs(np.asarray(weights[v], np.float64).ravel() - np.asarray(ref_weights[v], np.float64).ravel())
        out[f"adam{v}"] = float(d.max() / (2e-7 * steps))
        off += n
    return out


def own_adam_ratio(flat_grads, norms, before, after, hp, t):
    """k_adam alone: adam_step on the product's own gradients, norms and state before = (weights, m, v) at iteration t
    against its weights after, error / bound.  Bound per weight, derived: 2^-23 |w| (the last subtraction rounds once,
    on either side of a tie) + 8 * 2^-24 |update| (ballgame.hip is built with contraction on: a fused multiply-add
    changes m, v and so the update alpha m / (sqrt(v) + eps) by a few roundings of it) + 1e-12."""
    worst, off = 0.0, 0
    for v, n in enumerate(VAR_SIZES):
        w0 = np.asarray(before[0][v], np.float32).ravel()
        w, _, _ = adam_step(flat_grads[off:off + n], norms[v], w0, before[1][v].ravel(), before[2][v].ravel(), hp, t)
        got = np.asarray(after[v], np.float64).ravel()
        bound = 2.0 ** -23 * np.abs(got) + 8 * 2.0 ** -24 * np.abs(got - w0) + 1e-12
        worst = max(worst, float((np.abs(got - w) / bound).max()))
        off += n
    return worst


def worst_adam_element(flat_grads, weights, ref_grads, ref_weights):
    """'var v[i]: |w - w_ref|, g, g_ref' of the weight that differs most after the step (for the tests' printed line)."""
    best, off = (-1.0, ""), 0
    for v, n in enumerate(VAR_SIZES):
        d = np.abs(np.asarray(weights[v], np.float64).ravel() - np.asarray(ref_weights[v], np.float64).ravel())
        i = int(d.argmax())
        best = max(best, (float(d[i]), f"var {v}[{i}]: |w - w_ref| {d[i]:.3e}, g {flat_grads[off + i]:.6e}, "
                                       f"g_ref {np.asarray(ref_grads[v]).ravel()[i]:.6e}"))
        off += n
    return best[1]
