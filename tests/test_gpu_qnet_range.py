"""The Q-net's HIP kernels at the edges of the float32 range: subnormals, signed zeros, inf and NaN.

1. The update tail (clip_by_norm + Adam) over the regimes of tests/range_cases.py, one per variable, every rotation, three
   consecutive steps, scale 1 and 1 / 3 (DeepQLearningModel.apply_gradient on slots set with set(v, arr, which)):
   fp32 against oracle.qnet32_apply on a twin - the ten norms and w / m / v of all ten variables, NaNs at the same positions
   and every other element equal as uint32;
   bf16 against bf16_checks.adam_step fed the GPU's norms, the same comparison; the norms exactly 0, inf or NaN where the
   table says so, and every finite one within tests/test_gpu_qnet_bf16_update.py's 1e-5 of the float64 norm (regime b
   apart, whose float32 squares all underflow: its norm is exactly 0).
   tests/test_oracle_range.py holds the two references to each other on the CPU.  A NaN norm makes its whole variable NaN
   (the reference graph's Maximum, the oracle's std::max): with fmaxf in the kernels only the NaN element went bad.
2. A caller's dq (TorchQNet.backward_dq, both archs, B = 33): the gradient buffer of dq 2^24 is 2^24 times the buffer of dq,
   bit for bit - scaling by a power of two commutes with every rounding while nothing overflows or is subnormal - with
   whole rows of 0.0 and of -0.0 in dq; an all-zero dq gives a buffer that is zero everywhere.  No reference needed: an
   absolute threshold or clamp on that path would break the identity.
3. The fp32 chain (forward, backward, clip, Adam) through the subnormal range, bit for bit against the oracle: see
   test_fp32_chain_through_the_subnormal_range.
"""
import ctypes

import numpy as np
import pytest

import qlx_torch as QT   # before any other use of qlx in this process (it checks that itself)

import bf16_checks as C
import oracle as O
import range_cases as R
from test_gpu_qnet32 import mixed_states, randomize
from test_gpu_model_grad import DEV, LAY, dev, grads_host, pool   # noqa: F401 (pool: the fixture of 520 env states)

pytestmark = pytest.mark.gpu

CASES = [(rot, scale) for rot in range(len(R.ROTATIONS)) for scale in R.SCALES]


def _qlx():
    import qlx
    return qlx


def prepared(rotation, precision, twin=None):
    """a model (and the oracle twin) with non-zero biases and the rotation's Adam slots"""
    qlx = _qlx()
    m = qlx.DeepQLearningModel(seed=2, precision=precision)
    _, m0, v0 = R.draw(rotation, 1)
    for v, w in enumerate(C.nonzero_biases(m.weights(), 7)):
        for net in (m, twin) if twin is not None else (m,):
            net.set(v, w)
            net.set(v, m0[v], 1)
            net.set(v, v0[v], 2)
    return m


def slots(net):
    return [[net.get(v, which).ravel() for which in range(3)] for v in range(10)]


def differing(got, want):
    """description of where two arrays differ by same_bits' measure"""
    got, want = np.asarray(got, np.float32).ravel(), np.asarray(want, np.float32).ravel()
    ng, nw = np.isnan(got), np.isnan(want)
    bad = np.flatnonzero((ng != nw) | (~ng & ~nw & (got.view(np.uint32) != want.view(np.uint32))))
    return f"{bad.size} of {got.size} differ (NaN: {int(ng.sum())} got, {int(nw.sum())} wanted), first at {bad[:4]}: " \
           f"got {got[bad[:4]]}, wanted {want[bad[:4]]}"


@pytest.mark.parametrize("rotation,scale", CASES)
def test_fp32_update_tail_at_the_range_edges(rotation, scale):
    ref = O.QNet(seed=2, f32=True)
    m = prepared(rotation, _qlx().PREC_F32, ref)
    for v, (a, b) in enumerate(zip(slots(m), slots(ref))):
        assert all(R.same_bits(a[which], b[which]) for which in range(3)), f"var {v} before the first step"
    for t in range(1, R.STEPS + 1):
        flat = np.concatenate(R.draw(rotation, t)[0])
        got = m.apply_gradient(flat, scale)
        want = O.qnet32_apply(ref, flat, scale)
        tag = f"rotation {rotation} scale {scale:.3f} step {t}"
        print(f"{tag}: norms {got}")
        R.check_exact_norms(rotation, want, scale)
        assert R.same_bits(got, want), f"{tag}: norms {got} vs the oracle's {want}"
        for v, (a, b) in enumerate(zip(slots(m), slots(ref))):
            for which in range(3):
                assert R.same_bits(a[which], b[which]), \
                    f"{tag}: var {v} (regime {R.ROTATIONS[rotation][v]}) {'wmv'[which]}: " + differing(a[which], b[which])
        assert m.iterations() == ref.iterations() == t


@pytest.mark.parametrize("rotation,scale", CASES)
def test_bf16_update_tail_at_the_range_edges(rotation, scale):
    qlx = _qlx()
    m = prepared(rotation, qlx.PREC_BF16)
    hp = qlx.model_hparams()
    for t in range(1, R.STEPS + 1):
        grads = R.draw(rotation, t)[0]
        before = slots(m)
        norms = m.apply_gradient(np.concatenate(grads), scale)
        tag = f"rotation {rotation} scale {scale:.3f} step {t}"
        print(f"{tag}: norms {norms}")
        R.check_exact_norms(rotation, norms, scale)
        with np.errstate(all="ignore"):
            for v, r in enumerate(R.ROTATIONS[rotation]):
                if r not in R.EXACT_NORM:
                    want = np.sqrt(((grads[v].astype(np.float64) * np.float64(np.float32(scale))) ** 2).sum())
                    assert np.isfinite(norms[v]) and abs(norms[v] - want) <= 1e-5 * want, f"{tag}: norm of var {v} ({r}): {norms[v]} vs {want}"
            after = slots(m)
            for v, r in enumerate(R.ROTATIONS[rotation]):
                want = C.adam_step(grads[v], norms[v], *before[v], hp, t, np.float32(scale))
                for which in range(3):
                    assert R.same_bits(after[v][which], want[which]), \
                        f"{tag}: var {v} (regime {r}) {'wmv'[which]}: " + differing(after[v][which], want[which])
        assert m.iterations() == t


# ---------------------------------------------------------------- 2. a caller's dq scaled by a power of two

@pytest.mark.parametrize("arch", ["f32", "bf16"])
def test_backward_dq_scales_by_a_power_of_two(pool, arch):
    B = 33
    x = dev(pool[:B])
    net = QT.TorchQNet(arch, seed=5, device=DEV, reserve=64)
    dq = (np.random.default_rng(33).standard_normal((B, 3)) / B).astype(np.float32)
    dq[[2, 16, 32]] = 0.0    # whole rows of 0.0 (the last row of the ragged head block among them)
    dq[[5, 17]] = -0.0       # and of -0.0
    net.q(x, layout=LAY, want="q")
    ticket = net.forward_ticket()

    def buffer(d):
        net.backward_dq(dev(d), ticket, x, layout=LAY)
        net.discard_grad()
        return [g.copy() for g in grads_host(net)]

    small, big, zero = buffer(dq), buffer(dq * np.float32(2.0 ** 24)), buffer(np.zeros((B, 3), np.float32))
    assert net.forward_ticket() == ticket
    for v in range(10):
        assert np.isfinite(big[v]).all() and small[v].any(), v
        tiny = np.abs(small[v][small[v] != 0]).min()
        assert tiny >= R.TINY, f"var {v}: a subnormal gradient element ({tiny}): the identity does not have to hold"
        want = small[v] * np.float32(2.0 ** 24)
        assert R.same_bits(big[v], want), f"{arch} var {v}: {int((big[v] != want).sum())} of {want.size} elements differ"
        assert not zero[v].any(), f"{arch} var {v}: {np.count_nonzero(zero[v])} non-zero elements from an all-zero dq"
    net.sync()
    net.close()


# ---------------------------------------------------------------- 3. the fp32 chain through the subnormal range

CHAIN_K = 60
# layer pair -> (s, kernel and bias of layer L, kernel of layer L + 1, index of a_L)
CHAIN_PAIRS = {"conv1-conv2": (61, 0, 1, 2, 0), "conv3-fc1": (64, 4, 5, 6, 2), "fc1-fc2": (66, 6, 7, 8, 3)}
PER_SAMPLE = (12800, 5184, 3136, 512)


def share_subnormal(a):
    """(share of the non-zero elements that are subnormal, number of non-zero elements)"""
    nz = int(np.count_nonzero(a))
    return int(R.subnormal(a).sum()) / max(nz, 1), nz


@pytest.mark.parametrize("B", [5, 37])
@pytest.mark.parametrize("pair", list(CHAIN_PAIRS))
def test_fp32_chain_through_the_subnormal_range(pair, B):
    """Layer L's kernel and bias times 2^-s, layer L + 1's kernel times 2^+s (powers of two: the same weights reach the
    model and the oracle, and in exact arithmetic Q does not change), so a_L and the gradients flowing back through layer
    L + 1 pass through the subnormal range.  On weights of ordinary size no s can hold the norms finite: layer L's gradient
    grows by 2^s, and with the s ~ 124 that makes a_L subnormal its squares overflow (measured on the oracle: the norms of
    layer L's kernel and bias are inf for all three pairs).  So the net the recipe is applied to is test_gpu_qnet32's
    randomize() with conv1's kernel and every bias times 2^-k, k = 60: every activation, Q and (with targets y = q_a +
    2^-k N(0, 1.5)) every dq is exactly 2^-k times the ordinary net's, about 1e-18, the weight gradients (activation times
    dz) fall to 1e-40 and the loss to 1e-36, and s ~ 60 more takes a_L below 2^-126.

    s was chosen on the CPU from the oracle alone, as the smallest at which a quarter of a_L's non-zero elements are
    subnormal at one of the two batches.  Measured on the oracle (share of the non-zero elements that are subnormal;
    B = 5 / B = 37), Q, loss and all ten norms finite in every case:
        conv1-conv2  s = 61   a1 0.268 of 25,318 / 0.261 of 189,491   gradient of W3 0.73 / 0.91, of W2 0.27 / 0.41
        conv3-fc1    s = 64   a3 0.252 of 7,730 / 0.310 of 57,634     gradient of W1 0.31 / 0.42
        fc1-fc2      s = 66   a4 0.291 of 1,237 / 0.236 of 9,214      gradient of W1 0.31 / 0.42, of W2 0.27 / 0.41
    (layer L + 1's kernel gradient, a_L times a dz of 1e-20, underflows to zero everywhere.)  The test asserts at least 10 %
    for a_L and for one gradient variable, on the oracle's output, before it looks at the GPU's; then activations, Q, loss,
    gradients, norms and w / m / v after Adam are compared as test_forward_bit_exact and test_train_step_bit_exact do.

    First run on an MI355X: everything equal but, for conv3-fc1, the sign of zeros in the gradient of W3 (every product
    underflows there): 323,071 (B = 5) and 372,076 (B = 37) of 1,605,632 elements +0 on the GPU and -0 in the oracle.  The
    kernel's chain takes every term over whole 32-sample slabs, zeros past B, and a +0 product turns a -0 accumulator into
    +0; the oracle skipped the terms with a3 = 0 and stopped at B.  oracle/qnet32_ref.cpp now restates the kernel's chain."""
    qlx = _qlx()
    f = np.float32
    s, kl, bl, kn, layer = CHAIN_PAIRS[pair]
    m = qlx.DeepQLearningModel(seed=11)
    ref = O.QNet(seed=11, f32=True)
    randomize(m, ref, 11)
    ws = ref.weights()
    down = f(2.0 ** -CHAIN_K)
    for v in (0, 1, 3, 5, 7, 9):
        ws[v] = ws[v] * down
    ws[kl], ws[bl], ws[kn] = ws[kl] * f(2.0 ** -s), ws[bl] * f(2.0 ** -s), ws[kn] * f(2.0 ** s)
    for v in range(10):
        assert ws[v].dtype == f and np.isfinite(ws[v]).all()
        m.set(v, ws[v])
        ref.set(v, ws[v])
    x = mixed_states(B, B)
    rng = np.random.default_rng(B)
    a = rng.integers(0, 3, B).astype(np.uint8)
    qr, acts = ref.forward(x, acts=True)
    y = (qr[np.arange(B), a] + down * rng.normal(0, 1.5, B).astype(f)).astype(f)
    twin = O.QNet(seed=11, f32=True)   # the oracle's train on a copy: ref keeps the weights for the GPU's train
    for v in range(10):
        twin.set(v, ws[v])
    loss_r, grads_r, norms_r = twin.train(x, a, y)
    # the conditions, on the oracle's output alone
    share_a, nz_a = share_subnormal(acts[layer])
    shares_g = [share_subnormal(g)[0] for g in grads_r]
    print(f"{pair} B={B}: a{layer + 1} subnormal share {share_a:.3f} of {nz_a}; gradients {np.round(shares_g, 2)}; "
          f"loss {loss_r:.3e}; norms {norms_r}")
    assert share_a >= 0.10 and max(shares_g) >= 0.10
    assert np.isfinite(qr).all() and np.isfinite(loss_r) and np.isfinite(norms_r).all()
    # forward
    q, act = m.q_values(x)
    for l in range(4):
        got = np.zeros(B * PER_SAMPLE[l], f)
        assert qlx.lib().qlx_model_last_activation(m.h, l + 1, got.ctypes.data_as(ctypes.c_void_p)) == 0
        assert R.same_bits(got, acts[l]), f"a{l + 1}: " + differing(got, acts[l])
    assert R.same_bits(q, qr), differing(q, qr)
    assert np.array_equal(act, np.argmax(qr, axis=1))
    # train
    loss, grads, norms = m.train(x, a, y, want_grads=True)
    assert R.same_bits(f(loss), f(loss_r)), (loss, loss_r)
    for v in range(10):
        assert R.same_bits(grads[v], grads_r[v]), f"gradient of var {v}: " + differing(grads[v], grads_r[v])
    assert R.same_bits(norms, norms_r), (norms, norms_r)
    for v in range(10):
        for which in range(3):
            assert R.same_bits(m.get(v, which), twin.get(v, which)), \
                f"var {v} {'wmv'[which]} after Adam: " + differing(m.get(v, which), twin.get(v, which))
    assert m.iterations() == twin.iterations() == 1
