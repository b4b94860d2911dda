"""The snapshot frame codec on the GPU (frame_codec.hip) through its test hook qlx_frame_codec_roundtrip: frames are
packed on the device, brought to the host, sent back and unpacked.  For every frame count (one frame, a few, one more
than a chunk, two chunks and a ragged third) and every kind of frame, the unpacked frames equal the input, the packed
bytes equal the numpy restatement (tests/snapshot_reference.py) byte for byte, and their number is the formula 882 + nnz
per frame plus each chunk's header and nnz table.  The RAW codec round-trips as well."""
import numpy as np
import pytest

import snapshot_reference as R

pytestmark = pytest.mark.gpu

C = R.CHUNK_FRAMES
FB = R.FRAME_BYTES
COUNTS = [1, 3, C + 1, 2 * C + 5]
KINDS = ["zero", "full", "first_byte", "last_byte", "density_0.1", "density_1.0", "env"]


def _qlx():
    import qlx
    return qlx


@pytest.fixture(scope="module")
def env_frames():
    """2 C + 8 ring frames of Breakout envs in mid-episode (the reference tensor view, one 84 x 84 image per slot)"""
    qlx = _qlx()
    n_envs = (2 * C + 8) // 4
    env = qlx.BreakoutEnvironment(n_envs, seed=0x51A5EED)
    rng = np.random.default_rng(5)
    try:
        for _ in range(12):
            env.step(rng.integers(0, 3, n_envs))
        state = env.state()
    finally:
        env.close()
    frames = np.ascontiguousarray(state.transpose(0, 3, 1, 2)).reshape(-1, FB)
    frames.setflags(write=False)
    density = np.count_nonzero(frames) / frames.size
    assert 0.02 < density < 0.3 and len(np.unique(frames)) <= 8, (density, np.unique(frames))
    return frames


def make_frames(kind, n, env_frames, seed=1):
    rng = np.random.default_rng(seed)
    if kind == "zero":
        return np.zeros((n, FB), np.uint8)
    if kind == "full":
        return rng.integers(1, 256, (n, FB)).astype(np.uint8)   # the worst case: nnz = 7,056 in every frame
    if kind == "first_byte":
        f = np.zeros((n, FB), np.uint8)
        f[:, 0] = 1 + np.arange(n) % 255
        return f
    if kind == "last_byte":
        f = np.zeros((n, FB), np.uint8)
        f[:, FB - 1] = 255 - np.arange(n) % 255
        return f
    if kind == "density_0.1":
        return np.where(rng.random((n, FB)) < 0.1, rng.integers(1, 256, (n, FB)), 0).astype(np.uint8)
    if kind == "density_1.0":
        return rng.integers(0, 256, (n, FB)).astype(np.uint8)   # random bytes: 255 of 256 non-zero
    assert kind == "env"
    return np.array(env_frames[:n])


def check_bitmap(frames):
    qlx = _qlx()
    packed, out = qlx.frame_codec_roundtrip(frames, qlx.FRAME_CODEC_BITMAP)
    assert out.shape == frames.shape and np.array_equal(out, frames)
    n = frames.shape[0]
    chunks = [min(C, n - i) for i in range(0, n, C)]
    formula = sum(882 + int(np.count_nonzero(f)) for f in frames) + sum(8 + ((2 * m + 7) & ~7) for m in chunks)
    assert packed.size == formula == R.packed_size(frames)
    ref = R.pack(frames)
    assert packed.size == ref.size and np.array_equal(packed, ref)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", COUNTS)
def test_bitmap_roundtrip(n, kind, env_frames):
    check_bitmap(make_frames(kind, n, env_frames))


def test_bitmap_mixed_frames_across_chunks(env_frames):
    """every kind of frame in one stream, shuffled, so that consecutive frames' value offsets are as uneven as they get"""
    n = 2 * C + 5
    parts = [make_frames(k, n // len(KINDS) + 1, env_frames, seed=3) for k in KINDS]
    frames = np.concatenate(parts)[:n]
    frames = frames[np.random.default_rng(9).permutation(n)]
    check_bitmap(np.ascontiguousarray(frames))


@pytest.mark.parametrize("n", [1, 3, C + 1])
def test_raw_roundtrip(n, env_frames):
    qlx = _qlx()
    frames = np.concatenate([make_frames("env", n, env_frames), make_frames("density_0.1", n, env_frames)])[1:n + 1]
    frames = np.ascontiguousarray(frames)
    packed, out = qlx.frame_codec_roundtrip(frames, qlx.FRAME_CODEC_RAW)
    assert np.array_equal(out, frames)
    assert packed.size == n * FB and np.array_equal(packed, frames.reshape(-1))


def test_bad_arguments():
    qlx = _qlx()
    with pytest.raises(qlx.QlError, match="status -1"):
        qlx.frame_codec_roundtrip(np.zeros((2, FB), np.uint8), codec=7)
