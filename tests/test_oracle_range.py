"""The two references of the Q-net's update tail agree at the edges of float32 (tests/range_cases.py), on the CPU.

oracle.qnet32_apply (oracle/qnet32_ref.cpp, compiled C++) against bf16_checks.adam_step (numpy float32, one rounded operation
per line) fed the oracle's own norms: w, m and v of all ten variables, NaNs at the same positions and every other element
equal as uint32, over every rotation, three consecutive steps and both scales.  Neither flushes subnormals, and both let a
NaN norm through max(norm, clipnorm); so a GPU failure in tests/test_gpu_qnet_range.py is not an artefact of a reference.

The regimes are checked to be reached: non-zero subnormal elements in m and in v after a step, a norm of exactly 0, of exactly
1, of inf, a subnormal sum of squares, and a NaN norm with its whole variable NaN in all three slots.
"""
import numpy as np
import pytest

import bf16_checks as C
import oracle as O
import range_cases as R


def test_rotations_cover_the_paths():
    R.check_rotations()
    assert len(R.ROTATIONS) >= 3 and R.STEPS == 3 and R.SCALES == (1.0, 1.0 / 3.0)
    for n in R.VAR_SIZES:
        p = R.special_positions(n)
        assert p[0] == 0 and p[-1] == n - 1 and p.max() < n
        if n > 1024:
            assert {1023, 1024}.issubset(p.tolist()) and {3, 4}.issubset(p.tolist())
        if n >= 8192:
            assert len(set((p % 64).tolist())) == 64


def test_same_bits():
    f = np.float32
    nan2 = np.array([0x7FC00001], np.uint32).view(f)   # another NaN payload
    assert R.same_bits([1.0, np.nan, -0.0], [1.0, nan2[0], -0.0])
    assert not R.same_bits([0.0], [-0.0])
    assert not R.same_bits([np.nan, 1.0], [1.0, np.nan])
    assert not R.same_bits([1.0], [np.nextafter(f(1), f(2))])
    assert not R.same_bits([1.0], [1.0, 1.0])
    assert R.same_bits(f(1e-45), f(1e-45)) and not R.same_bits(f(1e-45), f(0))


def model_slots(net):
    return [[net.get(v, which).ravel() for which in range(3)] for v in range(10)]


@pytest.mark.parametrize("scale", R.SCALES)
@pytest.mark.parametrize("rotation", range(len(R.ROTATIONS)))
def test_oracle_equals_numpy_restatement(rotation, scale):
    net = O.QNet(seed=2, f32=True)
    hp = net.hparams()
    assert hp[4] == 1.0   # clipnorm: regimes d and e sit on it
    for v, w in enumerate(C.nonzero_biases(net.weights(), 7)):
        net.set(v, w)
    _, m0, v0 = R.draw(rotation, 1)
    for v in range(10):
        net.set(v, m0[v], 1)
        net.set(v, v0[v], 2)
    var = lambda r: R.variable_of(rotation, r)
    for t in range(1, R.STEPS + 1):
        grads = R.draw(rotation, t)[0]
        before = model_slots(net)
        norms = O.qnet32_apply(net, np.concatenate(grads), scale)
        assert net.iterations() == t
        R.check_exact_norms(rotation, norms, scale)
        after = model_slots(net)
        with np.errstate(all="ignore"):
            for v in range(10):
                want = C.adam_step(grads[v], norms[v], *before[v], hp, t, np.float32(scale))
                for which in range(3):
                    assert R.same_bits(after[v][which], want[which]), \
                        f"rotation {rotation} scale {scale:.3f} t {t}: var {v} ({R.ROTATIONS[rotation][v]}) {'wmv'[which]}"
        # the regimes are reached
        sub = {r: [int(R.subnormal(after[var(r)][which]).sum()) for which in (1, 2)] for r in ("a", "b", "c")}
        print(f"rotation {rotation} scale {scale:.3f} t {t}: norms {norms}; subnormal (m, v) elements after the step: {sub}")
        assert sub["a"][0] > 0 and sub["a"][1] > 0, "regime a: no subnormal m / v"
        if t == 1:   # (later the slots carry the earlier steps)
            # (m = 0.1 g: zero where g is below five units of the last place, subnormal everywhere else)
            assert sub["b"][0] == np.count_nonzero(after[var("b")][1]) > R.VAR_SIZES[var("b")] // 2, "regime b: m not subnormal"
            assert sub["c"][1] > R.VAR_SIZES[var("c")] // 4, "regime c: few subnormal v"
        assert norms[var("b")] == 0.0 and not np.signbit(norms[var("b")])
        assert 0 < float(norms[var("c'")]) ** 2 < R.TINY, "regime c': the sum of squares is not subnormal"
        if scale == 1.0:
            assert norms[var("d")] == 1.0
            assert norms[var("e")] == np.nextafter(np.float32(1), np.float32(2))
        assert np.isposinf(norms[var("f")]) and np.isposinf(norms[var("i")])
        assert np.isnan(norms[var("h")])
        for which in range(3):
            assert np.isnan(after[var("h")][which]).all(), "regime h: a NaN norm did not poison the whole variable"
        if t == 1:
            for which in range(3):
                assert np.isnan(after[var("i")][which]).sum() == 1, "regime i: inf / inf in one element, 0 in the others"
            mf = before[var("f")][1]   # regime f: every clipped gradient is +-0, so m only decays
            assert R.same_bits(after[var("f")][1], mf + (-mf) * (np.float32(1.0) - hp[1]))
