"""The fp32 conv1 kernels with fewer vector instructions beside their MFMAs: the bits stay the oracle's.

k_conv1_fwd32 passes over the LDS reads, ballots and branches of a 4 x 4 output tile whose 20 x 20 pixel field holds no
marked block (it stores relu(0 + bias) there; exact, since each of the tile's step ballots is zero in every wave), and
addresses its frame reads and a1 stores as a lane part plus a wave-uniform part; k_conv1_wgrad32 addresses an operand
group (one output row, five steps) from a lane base; the conv2 / conv3 backward-data epilogues use 32-bit offsets.  This
file holds them to the oracle (oracle/qnet32_ref.cpp) bit for bit where those paths begin and end:

  batch sizes   1, 2 (one conv1 weight-gradient chunk, half and full), 3 (a chunk with one sample), 17, 33 (across the
                16-sample partial chunks), 65 (across a 64-row tile)
  frame sets    all zero (every group and tile clear), no zero pixel (nothing clear), env frames, and one non-zero pixel
                per sample placed so that exactly one group and one tile are live, in the first and in the last group,
                and in each right-wall tile (4, 9, 14, 19, 24)

each as one training step (forward, backward, apply): a1..a4, the loss, the clip norms, all ten gradients and w / m / v.
The same cases run in a child process under QLX_F32_BG=0 (no step masks: every group computed; the oracle's dense mode)
and under QLX_F32_C1_SKIP=0 (every step issued: no group or tile may be passed over), since the switches are read when a
model is created.  The chunk-size forward kernel (B = 2,049) gets one forward on env frames.  The dense conv2 / conv3
forward's ragged remainder tiles get B = 7 and 11 under QLX_F32_BG=0 with QLX_NUM_CUS=8.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as O
from test_gpu_qnet32 import env_states, randomize, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (1, 2, 3, 17, 33, 65)
KINDS = ("zero", "full", "env", "pixel")
WSEED = 2306
ACT = {1: 12800, 2: 5184, 3: 3136, 4: 512}

# (row, column) of the single pixel: which conv1 outputs see it (oh in {row // 4 - 1, row // 4}, ow likewise, inside 0..19)
PIXELS = ((0, 0),      # group 0 only, tile 0 only
          (83, 83),    # group 19 only, tile 24 only (right wall, last group)
          (1, 70),     # group 0 only, tile 4 only (right wall, first group)
          (24, 75),    # tile 9
          (40, 80),    # tile 14
          (56, 69),    # tile 19
          (82, 1),     # group 19 only, tile 20 only
          (3, 3),      # the last pixel of block (0, 0)
          (42, 42),    # the middle: two groups, one tile
          (31, 67))    # a corner of four tiles (oh 6, 7 x ow 15, 16)


def pixel_states(B):
    x = np.zeros((B, 84, 84, 4), np.uint8)
    for b in range(B):
        r, c = PIXELS[(b + B) % len(PIXELS)]
        x[b, r, c, b % 4] = 1 + (b * 37) % 255
    return x


def live_sets(x):
    """per sample: the live operand groups (output rows oh) and forward tiles, restated from the frames"""
    out = []
    for s in x:
        nz = (s != 0).any(axis=2)
        groups, tiles = set(), set()
        for oh in range(20):
            for ow in range(20):
                if nz[4 * oh:4 * oh + 8, 4 * ow:4 * ow + 8].any():
                    groups.add(oh)
                    tiles.add(5 * (oh // 4) + ow // 4)
        out.append((groups, tiles))
    return out


def states(B, kind):
    if kind == "zero":
        return np.zeros((B, 84, 84, 4), np.uint8)
    if kind == "full":
        return np.random.default_rng(B).integers(1, 256, size=(B, 84, 84, 4), dtype=np.uint8)
    if kind == "env":
        return env_states(B, seed=40 + B)
    return pixel_states(B)


class _W:
    def __init__(self):
        self.w = {}

    def set(self, v, w):
        self.w[v] = w


def _fresh_ref():
    ref = O.QNet(seed=7, f32=True)
    w = _W()
    randomize(w, ref, WSEED)
    return ref, w.w


def _expect(x, a, y, dense):
    ref, _ = _fresh_ref()
    e = {}
    _, acts = ref.forward(x, acts=True)
    for layer in range(1, 5):
        e[f"a{layer}"] = acts[layer - 1].ravel()
    O.lib().orc_qnet32_set_dense(int(dense))
    try:
        loss, grads, norms = ref.train(x, a, y)
    finally:
        O.lib().orc_qnet32_set_dense(0)
    e["loss"], e["norms"] = np.float32(loss), np.asarray(norms, np.float32)
    for v in range(10):
        e[f"g{v}"] = grads[v]
        for which in range(3):
            e[f"s{v}_{which}"] = ref.get(v, which)
    return e


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """inputs of every (B, kind), the weights, and the oracle's results in both modes - computed once"""
    d = tmp_path_factory.mktemp("issue")
    ref, w = _fresh_ref()
    inp, exp = {f"w{v}": w[v] for v in range(10)}, {}
    for B in BATCHES:
        for kind in KINDS:
            x = states(B, kind)
            rng = np.random.default_rng(7 * B + len(kind))
            a = rng.integers(0, 3, B).astype(np.uint8)
            q0 = ref.forward(x)
            y = (q0[np.arange(B), a] + rng.normal(0, 1.5, B)).astype(np.float32)
            k = f"{B}_{kind}"
            inp[f"x_{k}"], inp[f"a_{k}"], inp[f"y_{k}"] = x, a, y
            exp[k] = {dense: _expect(x, a, y, dense) for dense in (False, True)}
    path = str(d / "in.npz")
    np.savez(path, **inp)
    return d, path, inp, exp


def _check(got, want, what):
    for k, w in want.items():
        g = np.asarray(got[k])
        w = np.asarray(w, np.float32)
        assert g.size == w.size, f"{what}: {k}: size {g.size} vs {w.size}"
        bad = np.flatnonzero(g.ravel().view(np.uint32) != w.ravel().view(np.uint32))
        assert bad.size == 0, f"{what}: {k}: {bad.size} of {w.size} elements differ (first {bad[:5]})"


def _run_case(qlx, w, x, a, y):
    m = qlx.DeepQLearningModel(seed=7)
    for v in range(10):
        m.set(v, w[f"w{v}"])
    out = {}
    loss, grads, norms = m.train(x, a, y, want_grads=True)
    for layer in range(1, 5):
        got = np.zeros(ACT[layer] * x.shape[0], np.float32)
        assert qlx.lib().qlx_model_last_activation(m.h, layer, got.ctypes.data_as(ctypes.c_void_p)) == 0
        out[f"a{layer}"] = got
    out["loss"], out["norms"] = np.float32(loss), np.asarray(norms, np.float32)
    for v in range(10):
        out[f"g{v}"] = grads[v]
        for which in range(3):
            out[f"s{v}_{which}"] = m.get(v, which)
    return out


def test_pixel_set_covers_the_edges():
    """the crafted frames do hold the cases the kernels' guards turn on"""
    seen_groups, seen_tiles, single = set(), set(), 0
    for B in BATCHES:
        for groups, tiles in live_sets(pixel_states(B)):
            if len(groups) == 1 and len(tiles) == 1:
                single += 1
                seen_groups |= groups
                seen_tiles |= tiles
    assert single > 0 and {0, 19} <= seen_groups and {0, 4, 20, 24} <= seen_tiles
    wall = set()
    for _, tiles in live_sets(pixel_states(65)):
        wall |= tiles & {4, 9, 14, 19, 24}
    assert wall == {4, 9, 14, 19, 24}
    assert all(not g and not t for g, t in live_sets(states(3, "zero")))
    assert all(len(g) == 20 and len(t) == 25 for g, t in live_sets(states(3, "full")))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B", BATCHES)
def test_train_step_bit_exact(cases, B, kind):
    import qlx
    _, _, inp, exp = cases
    k = f"{B}_{kind}"
    got = _run_case(qlx, inp, inp[f"x_{k}"], inp[f"a_{k}"], inp[f"y_{k}"])
    _check(got, exp[k][False], k)


CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [sys.argv[3], sys.argv[3] + "/tests", sys.argv[3] + "/q-learning_amd"]
import qlx
from test_gpu_qnet32_issue import _run_case
d = np.load(sys.argv[1])
out = {}
for k in [f[2:] for f in d.files if f.startswith("x_")]:   # every case of the input file
    for name, v in _run_case(qlx, d, d[f"x_{k}"], d[f"a_{k}"], d[f"y_{k}"]).items():
        out[f"{k}__{name}"] = v
np.savez(sys.argv[2], **out)
"""


def _child(path, out, env):
    """the cases of the input file `path` in a child process under the switches `env` (they are read when a model is created)"""
    cenv = {k: v for k, v in os.environ.items() if not k.startswith("QLX_F32_") and k != "QLX_NUM_CUS"}
    cenv.update(env)
    r = subprocess.run([sys.executable, "-c", CHILD, path, out, ROOT], env=cenv, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(out)


@pytest.mark.parametrize("env", [{"QLX_F32_BG": "0"}, {"QLX_F32_C1_SKIP": "0"}],
                         ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()))
def test_null_step_masks_bit_exact(cases, env):
    """every case again without the forward's step masks / with every step issued (one child process per switch)"""
    d, path, _, exp = cases
    got = _child(path, str(d / ("out_" + "_".join(f"{k}{v}" for k, v in env.items()) + ".npz")), env)
    dense = env.get("QLX_F32_BG") == "0"
    for k, both in exp.items():
        want = both[dense]
        _check({n: got[f"{k}__{n}"] for n in want}, want, f"{env}: {k}")


def _balanced_whole_tiles(M, ncu):
    """f32_forward's split of a dense conv forward over M rows: whole 64-row tiles, or 0 for the plain grid"""
    t = M // 64
    whole = t - t % ncu
    return 0 if whole < ncu or M - whole * 64 > 32 * ncu else whole


def test_dense_remainder_tiles_bit_exact(tmp_path):
    """The dense-frame conv2 / conv3 forward's balanced grid with a ragged last 16-row remainder tile (RowShift), which
    256 CUs reach only from B = 203: under QLX_NUM_CUS=8, B = 7 gives conv2 (M = 567) 8 whole tiles plus 4 remainder tiles,
    the last with 7 live rows, and conv3 (M = 343) the plain ragged grid; B = 11 gives conv3 (M = 539) 8 whole tiles plus 2
    remainder tiles, the last with 11 rows, and conv2 (M = 891) the plain ragged grid.  One training step each on env frames,
    QLX_F32_BG=0 and QLX_NUM_CUS=8 together in one child process, against the oracle's dense mode."""
    assert _balanced_whole_tiles(7 * 81, 8) == 8 and (7 * 81 - 512) % 16 == 7 and _balanced_whole_tiles(7 * 49, 8) == 0
    assert _balanced_whole_tiles(11 * 49, 8) == 8 and (11 * 49 - 512) % 16 == 11 and _balanced_whole_tiles(11 * 81, 8) == 0
    ref, w = _fresh_ref()
    inp, exp = {f"w{v}": w[v] for v in range(10)}, {}
    for B in (7, 11):
        x = env_states(B, seed=40 + B)
        rng = np.random.default_rng(7 * B)
        a = rng.integers(0, 3, B).astype(np.uint8)
        y = (ref.forward(x)[np.arange(B), a] + rng.normal(0, 1.5, B)).astype(np.float32)
        inp[f"x_{B}"], inp[f"a_{B}"], inp[f"y_{B}"] = x, a, y
        exp[B] = _expect(x, a, y, True)
    path = str(tmp_path / "in.npz")
    np.savez(path, **inp)
    got = _child(path, str(tmp_path / "out.npz"), {"QLX_F32_BG": "0", "QLX_NUM_CUS": "8"})
    for B, want in exp.items():
        _check({n: got[f"{B}__{n}"] for n in want}, want, f"dense, 8 CUs: B = {B}")


def test_chunk_form_forward_bit_exact():
    """B = 2,049: the chunk-size conv1 forward (several samples per block, the row masks rotating through three buffers)"""
    import qlx
    B = 2049
    m = qlx.DeepQLearningModel(seed=7)
    ref, w = _fresh_ref()
    for v in range(10):
        m.set(v, w[v])
    x = env_states(B, seed=77)
    q, _ = m.q_values(x)
    qr, acts = ref.forward(x, acts=True)
    for layer in range(1, 5):
        got = np.zeros(ACT[layer] * B, np.float32)
        assert qlx.lib().qlx_model_last_activation(m.h, layer, got.ctypes.data_as(ctypes.c_void_p)) == 0
        bad = np.flatnonzero(got.view(np.uint32) != acts[layer - 1].ravel().view(np.uint32))
        assert bad.size == 0, f"layer {layer}: {bad.size} elements differ, first {bad[:5]}"
    assert same(q, qr)
