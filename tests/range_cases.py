"""Range regimes for the Q-net's update tail (clip_by_norm + Adam): gradients and Adam slots at the edges of float32.

The clip norm is per variable, so one call to the tail runs ten regimes at once, one per variable.  A regime is a function of
(variable size n, rng) returning (gradient, m slot, v slot) as float32 arrays of n elements:

    a   gradient 0; m (signed) and v spread over 1e-45 .. 1e-36: slots decaying through the subnormal range and out to zero
    b   gradient subnormal (1e-45 .. 1e-38), slots 0: every square underflows, the norm is exactly 0 (the t > 0 ? sqrt : t
        branch), m is subnormal afterwards
    c   gradient about 1e-20, slots 0: subnormal squares, v subnormal afterwards
    c'  gradient +-3 k 2^-72 (k = 1, 2, 3: about 1e-21) on a small variable, slots 0: the sum of squares is subnormal, so sqrtf
        of a subnormal.  Every square (9 k^2 2^-144) and, the subnormal range being fixed-point, every partial sum is exact
        in float32 whatever the order; under scale = float32(1 / 3) the scaled element is exactly k 2^-72 (3 k (2^25 + 1)
        2^-25 rounds to k), so the norm is the correctly rounded square root of an exact sum at both scales
    d   one 1.0, the rest 0, slots 0: norm == clipnorm exactly (scale 1)
    e   one nextafter(1, 2), the rest 0, slots 0: the norm just above clipnorm
    f   gradient 1e17 .. 1e20 (one element 1e20), ordinary slots: the sum of squares overflows, norm inf, every clipped
        gradient 0, the slots decay
    g   ordinary N(0, 1e-3) with every third element -0.0; ordinary slots but v == 0 and m == 1e-30 on special_positions:
        the sign of zero, sqrt(0) + eps
    h   ordinary with one NaN element, ordinary slots: a NaN norm, which makes the whole variable NaN in w, m and v
    i   ordinary with one +inf element, ordinary slots: norm inf, that element inf / inf = NaN, every other clipped to 0

Single special elements (d, e, h, i) sit on one of special_positions(n), drawn by the rng; so does every v == 0 of g.

ROTATIONS maps variable -> regime.  One rotation puts one regime on W3 (variable 6, the fp32 AdamDense path with 13 norm
partials per lane), and four regimes (a, f, h, i) must each meet W3, a conv kernel and a bias once: that takes four rotations,
not three.  check_rotations() asserts the coverage.
"""
import numpy as np

VAR_SIZES = (8192, 32, 32768, 64, 36864, 64, 1605632, 512, 1536, 3)
CONV_KERNELS, BIASES, W3 = (0, 2, 4), (1, 3, 5, 7, 9), 6
SCALES = (1.0, 1.0 / 3.0)
STEPS = 3
TINY = float(np.finfo(np.float32).tiny)   # the smallest normal float32

ROTATIONS = (
    ("a", "i", "c", "d", "g", "c'", "f", "h", "b", "e"),
    ("f", "a", "i", "c'", "c", "b", "h", "g", "e", "d"),
    ("g", "e", "b", "f", "h", "d", "a", "i", "c", "c'"),
    ("c", "b", "g", "e", "d", "a", "i", "c'", "h", "f"),
)
# the norm the table fixes exactly (at every scale; d's 1.0 holds at scale 1 only and is checked where it is needed)
EXACT_NORM = {"a": 0.0, "b": 0.0, "f": np.inf, "h": np.nan, "i": np.inf}


def special_positions(n):
    """Sorted positions of an n-element variable that every lane, the four-wide loads and the block tails meet: the first and
    last element, both sides of every multiple of 1,024, both sides of every 37th multiple of 4 (4 + 148 j: every multiple
    of 4 modulo 64) and every 61st element (61 is odd: every residue modulo 64)."""
    p = {0, n - 1}
    for k in range(1024, n, 1024):
        p.update((k - 1, k))
    for k in range(4, n, 4 * 37):
        p.update((k - 1, k))
    p.update(range(0, n, 61))
    return np.array(sorted(p), np.int64)


def _signs(n, rng):
    return rng.choice([-1.0, 1.0], n)


def _log_uniform(n, rng, lo, hi):
    return 10.0 ** rng.uniform(lo, hi, n)


def _ordinary(n, rng):
    f = np.float32
    return rng.normal(0, 1e-3, n).astype(f), rng.normal(0, 1e-3, n).astype(f), rng.uniform(1e-8, 1e-5, n).astype(f)


def _zeros(n):
    return np.zeros(n, np.float32), np.zeros(n, np.float32)


def _one(n, rng, value):
    g = np.zeros(n, np.float32)
    g[rng.choice(special_positions(n))] = value
    return g


def regime_a(n, rng):
    m = (_signs(n, rng) * _log_uniform(n, rng, -45, -36)).astype(np.float32)
    return np.zeros(n, np.float32), m, _log_uniform(n, rng, -45, -36).astype(np.float32)


def regime_b(n, rng):
    g = (_signs(n, rng) * np.minimum(_log_uniform(n, rng, -45, -38), 0.99 * TINY)).astype(np.float32)
    assert (g != 0).all() and (np.abs(g) < TINY).all()
    return (g,) + _zeros(n)


def regime_c(n, rng):
    assert n >= 512, "regime c wants enough elements for the float64 norm to be within 1e-5 of the float32 one"
    return ((_signs(n, rng) * rng.uniform(0.5e-20, 2e-20, n)).astype(np.float32),) + _zeros(n)


def regime_c1(n, rng):
    assert n * 81 * 32 < 2 ** 23, "the sum of squares must stay subnormal"
    g = _signs(n, rng) * 3.0 * rng.integers(1, 4, n) * 2.0 ** -72
    return (g.astype(np.float32),) + _zeros(n)


def regime_d(n, rng):
    return (_one(n, rng, 1.0),) + _zeros(n)


def regime_e(n, rng):
    return (_one(n, rng, np.nextafter(np.float32(1), np.float32(2))),) + _zeros(n)


def regime_f(n, rng):
    g = (_signs(n, rng) * _log_uniform(n, rng, 17, 20)).astype(np.float32)
    g[rng.choice(special_positions(n))] = 1e20
    return (g,) + _ordinary(n, rng)[1:]


def regime_g(n, rng):
    g, m, v = _ordinary(n, rng)
    g[::3] = -0.0
    sp = special_positions(n)
    m[sp], v[sp] = 1e-30, 0.0
    return g, m, v


def regime_h(n, rng):
    g, m, v = _ordinary(n, rng)
    g[rng.choice(special_positions(n))] = np.nan
    return g, m, v


def regime_i(n, rng):
    g, m, v = _ordinary(n, rng)
    g[rng.choice(special_positions(n))] = np.inf
    return g, m, v


REGIMES = {"a": regime_a, "b": regime_b, "c": regime_c, "c'": regime_c1, "d": regime_d, "e": regime_e, "f": regime_f,
           "g": regime_g, "h": regime_h, "i": regime_i}


def check_rotations():
    for rot in ROTATIONS:
        assert sorted(rot) == sorted(REGIMES), rot
    for r in "afhi":
        where = [rot.index(r) for rot in ROTATIONS]
        assert W3 in where and set(where) & set(CONV_KERNELS) and set(where) & set(BIASES), (r, where)


def variable_of(rotation, regime):
    return ROTATIONS[rotation].index(regime)


def draw(rotation, t):
    """(gradients, m slots, v slots), each a list of ten float32 arrays, of step t (1, 2, 3) of a rotation.  The slots are
    set once, from draw(rotation, 1); the later steps use the gradients only."""
    out = [REGIMES[r](VAR_SIZES[v], np.random.default_rng([rotation, v, t])) for v, r in enumerate(ROTATIONS[rotation])]
    for g, m, s in out:
        assert g.dtype == m.dtype == s.dtype == np.float32
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]


def same_bits(a, b):
    """NaNs at the same positions and every other element equal as uint32 (so -0.0 is not 0.0)."""
    a = np.ascontiguousarray(np.atleast_1d(a), dtype=np.float32).ravel()
    b = np.ascontiguousarray(np.atleast_1d(b), dtype=np.float32).ravel()
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def subnormal(a):
    """mask of the non-zero subnormal elements"""
    a = np.abs(np.asarray(a, np.float32))
    return (a > 0) & (a < np.float32(TINY))


def check_exact_norms(rotation, norms, scale):
    """the norms the table fixes: exactly 0, inf or NaN (and exactly 1.0 for d at scale 1)"""
    for v, r in enumerate(ROTATIONS[rotation]):
        want = EXACT_NORM.get(r, 1.0 if r == "d" and scale == 1.0 else None)
        if want is not None:
            got = np.float32(norms[v])
            assert same_bits(got, np.float32(want)), f"rotation {rotation} regime {r} (var {v}): norm {got}, not {want}"
