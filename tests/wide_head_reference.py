"""Float64 numpy restatement of the wide output head (q-learning_amd/csrc/head_wide.hip), with the error
bounds its tests use.  The inputs are the float32 arrays the kernels read (the GPU's own a4 among them); every function
computes in float64 in the kernels' stated order and returns, beside the value, the sum of the absolute terms of each
output's chain, so that a test can form the standard bound

    |fl(chain) - exact| <= gamma(n) * sum |terms|,   gamma(n) = n u / (1 - n u),   u = 2^-24

for a chain of n rounded operations (Higham, Accuracy and Stability of Numerical Algorithms, §3.1: an fmaf chain of n
products rounds n times; the forward adds three partial sums and a bias on top of 128-step chains, 512 + 4 < 520).
"""
import numpy as np

U = 2.0 ** -24
HEAD_IN = 512
NORM_SEG = 2048   # clip_by_norm segment length (kNormSeg)


def gamma(n):
    return n * U / (1.0 - n * U)


def f64(a):
    return np.asarray(a, dtype=np.float64)


def forward(a4, wh, bh):
    """Z[b][j] = (((C0 + C1) + C2) + C3) + bh[j], Cw the chain over k ascending in [128 w, 128 w + 128) of a4[b][k] Wh[k][j]:
    (Z, sum of |terms|) for a4 [B, 512], Wh [512, width], bh [width]"""
    a4, wh, bh = f64(a4), f64(wh), f64(bh)
    z = np.zeros((a4.shape[0], wh.shape[1]))
    for w in range(4):
        k = slice(128 * w, 128 * w + 128)
        z = z + a4[:, k] @ wh[k]
    return z + bh, np.abs(a4) @ np.abs(wh) + np.abs(bh)


def backward_data(a4, wh, dz, w4=None, dq=None):
    """dz4[b][k] = a4[b][k] > 0 ? chain : 0; the chain runs over n = 0, 1, 2 of W4[k][n] dq[b][n] (with dq), then over j
    ascending of Wh[k][j] dz[b][j]: (dz4, sum of |terms|), n = width + 3 operations at the most"""
    a4, wh, dz = f64(a4), f64(wh), f64(dz)
    chain = np.zeros((a4.shape[0], HEAD_IN))
    terms = np.zeros_like(chain)
    if dq is not None:
        chain = chain + f64(dq) @ f64(w4).T
        terms = terms + np.abs(f64(dq)) @ np.abs(f64(w4)).T
    chain = chain + dz @ wh.T
    terms = terms + np.abs(dz) @ np.abs(wh).T
    mask = a4 > 0
    return np.where(mask, chain, 0.0), np.where(mask, terms, 0.0)


def weight_grads(a4, dz):
    """dWh[k][j] = chain over b ascending of a4[b][k] dz[b][j], dbh[j] the same with 1 for a4 (B + 1 operations at the
    most): (dWh, dbh, |terms| of dWh, |terms| of dbh)"""
    a4, dz = f64(a4), f64(dz)
    return a4.T @ dz, dz.sum(axis=0), np.abs(a4).T @ np.abs(dz), np.abs(dz).sum(axis=0)


def adam_alpha(hp, t):
    """Adam's step size of update t (1-based) as the host computes it, in float32: lr sqrt(1 - beta2^t) / (1 - beta1^t)"""
    f = np.float32
    lr, b1, b2 = f(hp[0]), f(hp[1]), f(hp[2])
    b1p, b2p = f(np.power(b1, f(t))), f(np.power(b2, f(t)))
    return f(f(lr * f(np.sqrt(f(f(1) - b2p)))) / f(f(1) - b1p))


def clip_adam(w, m, v, g, t, hp):
    """tf.clip_by_norm(g, clipnorm) + legacy ResourceApplyAdam of one variable at update t (1-based), in float64, from the
    float32 hyperparameters hp = (lr, beta1, beta2, eps, clipnorm): (w', m', v', norm).  The norm is the segment scheme's
    value up to rounding (a sum of squares in any order); 1 - beta is the float32 difference, which is exact."""
    w, m, v, g = f64(w), f64(m), f64(v), f64(g)
    b1, b2, eps, clip = (float(np.float32(x)) for x in hp[1:5])
    norm = np.sqrt(np.sum(g * g))
    gc = g * clip / max(norm, clip)
    m = m + (gc - m) * float(np.float32(1) - np.float32(b1))
    v = v + (gc * gc - v) * float(np.float32(1) - np.float32(b2))
    return w - m * float(adam_alpha(hp, t)) / (np.sqrt(v) + eps), m, v, norm
