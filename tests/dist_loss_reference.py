"""Restatements of the distributional losses on the wide head (include/qlx.h "distributional losses") that the
tests compare the HIP kernels against.  A head of width 3 N is read as Z[b][a N + i].

(a) quantile32 / values32: the quantile contract in numpy float32, operation for operation and in the kernels' stated
    orders (csrc/dist_loss.hip's head note); nothing there is fused, so the GPU must give the same bits.
(b) quantile64 / categorical64 / values64: both losses, the values and the gradients in float64, in the plain order numpy
    chooses.  categorical64 can also return a bound on the fp32 kernel's error for every output, propagated through the
    kernel's operations from u = 2^-24 per fp32 operation and ULPS ulp for expf / logf (see categorical64)."""
import numpy as np

F = np.float32
U = 2.0 ** -24      # unit roundoff of fp32
ULPS = 2            # expf / logf: counted as 2 ulp each (the ROCm math-function accuracy tables are not in the tree)
EXPLOG = ULPS * 2 * U   # ... as a relative error: one ulp is at most 2 u of the value
TINY = 2.0 ** -148  # absolute error of an expf result in the subnormal range (exp(-120) is flushed to 0 or a subnormal)
SLACK = 1.01        # covers the second-order terms the first-order propagation below drops


def gamma(n):
    return n * U / (1 - n * U)


def f64(a):
    return np.asarray(a, np.float64)


# ---------------------------------------------------------------------------------------------------------------- (a)

def wave_sum32(x):
    """S(x, n) over the last axis: lane l chains x[l], x[l + 64], .. ascending from +0; xor butterfly 32, 16, .., 1.
    (Padding with +0 changes no bit: a chain that started at +0 is never -0.)"""
    x = np.asarray(x, F)
    n = x.shape[-1]
    pad = (-n) % 64
    if pad or n == 0:
        x = np.concatenate([x, np.zeros(x.shape[:-1] + (pad if n else 64,), F)], axis=-1)
    acc = np.zeros(x.shape[:-1] + (64,), F)
    for k in range(x.shape[-1] // 64):
        acc = acc + x[..., 64 * k:64 * k + 64]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., lanes ^ o]
    return acc[..., 0]


def first_argmax(q):
    return np.argmax(q, axis=-1).astype(np.uint8)   # numpy's argmax is the first maximal index


def values32_quantile(z, N):
    """(Q [n, 3], first argmax, max-Q) of z [n, 3 N]: Q = S(row, N) / N"""
    z = np.asarray(z, F).reshape(-1, 3, N)
    q = wave_sum32(z) / F(N)
    a = first_argmax(q)
    return q, a, q[np.arange(len(q)), a]


def quantile32(z, actions, returns, discounts, terminals, z_next, N, a_star=None, weights=None):
    """dict(dz [B, 3 N], sample_loss [B], loss, a_star [B]) with the kernel's bits"""
    z = np.asarray(z, F).reshape(-1, 3, N)
    zn = np.asarray(z_next, F).reshape(-1, 3, N)
    B = len(z)
    rows = np.arange(B)
    act = np.where(np.asarray(actions) >= 3, 0, actions).astype(np.int64)
    if a_star is None:
        a_star = values32_quantile(zn, N)[1]
    a_star = np.where(np.asarray(a_star) >= 3, 0, a_star).astype(np.int64)
    ret = np.asarray(returns, F)
    live = np.where(np.asarray(terminals) != 0, F(0), np.asarray(discounts, F)).astype(F)
    w = np.ones(B, F) if weights is None else np.asarray(weights, F)
    T = ret[:, None] + live[:, None] * zn[rows, a_star]          # [B, N], two roundings
    theta = z[rows, act]
    tau = (np.arange(N, dtype=F) + F(0.5)) / F(N)
    wpos, wneg = np.abs(tau), np.abs(tau - F(1))
    sh, sg = np.zeros((B, N), F), np.zeros((B, N), F)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(N):
            u = T[:, j:j + 1] - theta
            au = np.abs(u)
            h = np.where(au <= F(1), (F(0.5) * u) * u, au - F(0.5))
            om = np.where(u < F(0), wneg, wpos)
            sh = sh + om * h
            sg = sg + om * np.where(u < F(-1), F(-1), np.where(u > F(1), F(1), u))
        Lb = wave_sum32(sh / F(N))
        dz = np.zeros((B, 3, N), F)
        dz[rows, act] = (w[:, None] * ((-sg) / F(N))) / F(B)
        loss = wave_sum32(w * Lb) / F(B)
    return dict(dz=dz.reshape(B, 3 * N), sample_loss=Lb.astype(F), loss=F(loss), a_star=a_star.astype(np.uint8))


# ---------------------------------------------------------------------------------------------------------------- (b)

def values64_quantile(z, N):
    q = f64(z).reshape(-1, 3, N).mean(axis=2)
    a = first_argmax(q)
    return q, a, q[np.arange(len(q)), a]


def quantile64(z, actions, returns, discounts, terminals, z_next, N, a_star=None, weights=None):
    z = f64(z).reshape(-1, 3, N)
    zn = f64(z_next).reshape(-1, 3, N)
    B = len(z)
    rows = np.arange(B)
    act = np.asarray(actions).astype(np.int64)
    if a_star is None:
        a_star = values64_quantile(zn, N)[1]
    a_star = np.asarray(a_star).astype(np.int64)
    live = np.where(np.asarray(terminals) != 0, 0.0, f64(discounts))
    w = np.ones(B) if weights is None else f64(weights)
    T = f64(returns)[:, None] + live[:, None] * zn[rows, a_star]
    theta = z[rows, act]
    tau = (np.arange(N) + 0.5) / N
    u = T[:, None, :] - theta[:, :, None]                       # [B, i, j]
    h = np.where(np.abs(u) <= 1, 0.5 * u * u, np.abs(u) - 0.5)
    om = np.abs(tau[None, :, None] - (u < 0))
    Lb = (om * h).sum(axis=2).sum(axis=1) / N
    dz = np.zeros((B, 3, N))
    dz[rows, act] = w[:, None] * (-(om * np.clip(u, -1, 1)).sum(axis=2) / N) / B
    return dict(dz=dz.reshape(B, 3 * N), sample_loss=Lb, loss=float((w * Lb).sum() / B), a_star=a_star.astype(np.uint8))


def atoms64(N, v_min, v_max):
    v_min, v_max = float(F(v_min)), float(F(v_max))
    delta = (v_max - v_min) / (N - 1)
    return v_min + np.arange(N) * delta, delta


def _softmax_rows(x, zk, ez):
    """rows x [..., N] in float64: (p, S, mx, Q) and the fp32 kernel's error bounds (rel_e [..., N] of each exp, err_S,
    err_Q); zk the atoms, ez their error"""
    mx = x.max(axis=-1, keepdims=True)
    d = x - mx
    e = np.exp(d)
    S = e.sum(axis=-1, keepdims=True)
    rel_e = np.abs(d) * U + EXPLOG                    # the rounded subtraction moves the argument by u |d|
    err_e = rel_e * e + TINY
    err_S = err_e.sum(axis=-1, keepdims=True) + gamma(12) * S        # S(): at most 6 chain steps + 6 butterfly levels
    num = (e * zk).sum(axis=-1, keepdims=True)
    abs_num = (e * np.abs(zk)).sum(axis=-1, keepdims=True)
    err_num = (err_e * np.abs(zk) + e * ez + U * e * np.abs(zk)).sum(axis=-1, keepdims=True) + gamma(12) * abs_num
    Q = num / S
    err_Q = err_num / S + np.abs(num) * err_S / S ** 2 + U * np.abs(Q)
    return e / S, S, mx, Q[..., 0], rel_e, err_S, err_Q[..., 0]


def values64_categorical(z, N, v_min, v_max, bounds=False):
    """(Q [n, 3], first argmax, max-Q[, err_Q [n, 3]]) of z [n, 3 N]"""
    zk, delta = atoms64(N, v_min, v_max)
    ez = 3 * U * np.arange(N) * delta + U * np.abs(zk)
    _, _, _, q, _, _, err_q = _softmax_rows(f64(z).reshape(-1, 3, N), zk, ez)
    a = first_argmax(q)
    out = (q, a, q[np.arange(len(q)), a])
    return out + (SLACK * err_q,) if bounds else out


def project_gather(p_next, Tz, zk, delta):
    """m_i = sum_k p'_k max(0, 1 - |Tz_k - z_i| / delta) for rows [B, N]"""
    hat = np.maximum(0.0, 1.0 - np.abs(Tz[:, None, :] - zk[None, :, None]) / delta)   # [B, i, k]
    return (p_next[:, None, :] * hat).sum(axis=2)


def project_scatter(p_next, Tz, N, v_min, delta):
    """the classic C51 projection (Bellemare et al. 2017, Algorithm 1): mass p'_k to floor and ceil of (Tz_k - v_min) / delta;
    a Tz on an atom gives it all to that atom"""
    m = np.zeros_like(p_next)
    bj = (Tz - v_min) / delta
    lo, hi = np.floor(bj).astype(np.int64), np.ceil(bj).astype(np.int64)
    lo, hi = np.clip(lo, 0, N - 1), np.clip(hi, 0, N - 1)
    for b in range(len(m)):
        for k in range(N):
            if lo[b, k] == hi[b, k]:
                m[b, lo[b, k]] += p_next[b, k]
            else:
                m[b, lo[b, k]] += p_next[b, k] * (hi[b, k] - bj[b, k])
                m[b, hi[b, k]] += p_next[b, k] * (bj[b, k] - lo[b, k])
    return m


def categorical64(z, actions, returns, discounts, terminals, z_next, N, v_min, v_max, a_star=None, weights=None, bounds=False):
    """dict(dz, sample_loss, loss, a_star, m) in float64.  With bounds: also err_dz, err_sample_loss, err_loss, the fp32
    kernel's worst-case error for these inputs, propagated to first order through its operations (csrc/dist_loss.hip's head
    note) and multiplied by SLACK: every +, -, *, / rounds once (u); expf and logf are ULPS ulp; a sum S() is at most 12
    additions deep; the chain over k is N multiply-adds; the atoms carry the rounding of delta (two operations on the host),
    of k delta and of the addition; 1 / delta three roundings; max and clamp do not enlarge an error, and a hat whose
    argument stays above 1 by more than its error is 0 on both sides."""
    z = f64(z).reshape(-1, 3, N)
    zn = f64(z_next).reshape(-1, 3, N)
    B = len(z)
    rows = np.arange(B)
    zk, delta = atoms64(N, v_min, v_max)
    ez = 3 * U * np.arange(N) * delta + U * np.abs(zk)
    act = np.asarray(actions).astype(np.int64)
    if a_star is None:
        a_star = values64_categorical(zn, N, v_min, v_max)[1]
    a_star = np.asarray(a_star).astype(np.int64)
    live = np.where(np.asarray(terminals) != 0, 0.0, f64(discounts))
    ret = f64(returns)
    w = np.ones(B) if weights is None else f64(weights)
    pn, Sn, _, _, rel_en, err_Sn, _ = _softmax_rows(zn[rows, a_star], zk, ez)
    err_pn = pn * (rel_en + err_Sn / Sn + U) + TINY / Sn
    raw = ret[:, None] + live[:, None] * zk[None, :]
    Tz = np.clip(raw, zk[0], zk[-1])
    err_T = np.abs(live)[:, None] * (ez + U * np.abs(zk))[None, :] + U * np.abs(raw)
    x = z[rows, act]
    p, S, mx, _, _, err_S, _ = _softmax_rows(x, zk, ez)
    logS = np.log(S)
    lp = (x - mx) - logS
    err_lp = U * np.abs(x - mx) + err_S / S + EXPLOG * np.abs(logS) + TINY + U * np.abs(lp)
    m = np.zeros((B, N))
    err_m = np.zeros((B, N))
    for b in range(B):
        dist = np.abs(Tz[b][None, :] - zk[:, None])                       # [i, k]
        a = dist / delta
        hat = np.maximum(0.0, 1.0 - a)
        m[b] = (pn[b][None, :] * hat).sum(axis=1)
        if bounds:
            err_a = (err_T[b][None, :] + ez[:, None] + U * dist) / delta + 4 * U * a
            err_hat = np.where(a - err_a > 1.0, 0.0, err_a + U)
            err_m[b] = (err_pn[b][None, :] * hat + pn[b][None, :] * err_hat).sum(axis=1) + gamma(N + 1) * m[b]
    Lb = -(m * lp).sum(axis=1)
    M = m.sum(axis=1)
    dzr = w[:, None] * (p * M[:, None] - m) / B
    dz = np.zeros((B, 3, N))
    dz[rows, act] = dzr
    loss = float((w * Lb).sum() / B)
    out = dict(dz=dz.reshape(B, 3 * N), sample_loss=Lb, loss=loss, a_star=a_star.astype(np.uint8), m=m)
    if bounds:
        err_ml = err_m * np.abs(lp) + m * err_lp + U * np.abs(m * lp)
        err_L = err_ml.sum(axis=1) + gamma(12) * np.abs(m * lp).sum(axis=1)
        err_M = err_m.sum(axis=1) + gamma(12) * M
        rel_p = err_lp + EXPLOG
        pM = p * M[:, None]
        # (expf(log p) in the subnormal range, and a dz there, are off by an absolute TINY, not by a relative error)
        err_row = ((np.abs(w)[:, None] / B) * (pM * (rel_p + U) + TINY * M[:, None] + p * err_M[:, None] + err_m + U * np.abs(pM - m))
                   + 2 * U * np.abs(dzr) + 2 * TINY)
        err_dz = np.zeros((B, 3, N))
        err_dz[rows, act] = err_row
        depth = (B + 63) // 64 + 6
        err_loss = ((np.abs(w) * (err_L + U * np.abs(Lb))).sum() + gamma(depth) * np.abs(w * Lb).sum()) / B + U * abs(loss)
        out.update(err_dz=SLACK * err_dz.reshape(B, 3 * N), err_sample_loss=SLACK * err_L, err_loss=SLACK * float(err_loss))
    return out
