"""The numpy restatement of the bitmap frame codec (tests/snapshot_reference.py) against hand-made frames: the packed
bytes are spelled out from the definition (a plain per-byte loop), unpacking returns the input, and the size is the
formula 882 + nnz per frame plus each chunk's header and nnz table.  No GPU needed."""
import struct

import numpy as np
import pytest

import snapshot_reference as R

FB = R.FRAME_BYTES


def _frames():
    rng = np.random.default_rng(7)
    zero = np.zeros(FB, np.uint8)
    full = np.full(FB, 255, np.uint8)
    first = zero.copy(); first[0] = 9
    last = zero.copy(); last[FB - 1] = 200
    group = zero.copy(); group[16 * 5:16 * 6] = np.arange(1, 17)
    sparse = np.where(rng.random(FB) < 0.1, rng.integers(1, 256, FB), 0).astype(np.uint8)
    dense = rng.integers(1, 256, FB).astype(np.uint8)
    return dict(zero=zero, full=full, first=first, last=last, group=group, sparse=sparse, dense=dense)


FRAMES = _frames()


def _pack_by_definition(frames):
    """one chunk, byte by byte"""
    n = len(frames)
    nnz, masks, values = [], bytearray(), bytearray()
    for f in frames:
        mask = bytearray(R.MASK_BYTES)
        k = 0
        for i, v in enumerate(f.tolist()):
            if v:
                mask[i >> 3] |= 1 << (i & 7)
                values.append(v)
                k += 1
        nnz.append(k)
        masks += mask
    table = struct.pack("<%dH" % n, *nnz)
    table += bytes(-len(table) % 8)
    return struct.pack("<II", n, len(values)) + table + bytes(masks) + bytes(values)


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_single_frame(name):
    f = FRAMES[name][None]
    packed = R.pack(f)
    assert packed.tobytes() == _pack_by_definition(list(f))
    nnz = int(np.count_nonzero(f))
    assert packed.size == 8 + 8 + 882 + nnz == R.packed_size(f)
    assert np.array_equal(R.unpack(packed, 1), f)


def test_known_bytes():
    p = R.pack(FRAMES["first"][None])
    assert struct.unpack("<IIH", p[:10].tobytes()) == (1, 1, 1) and p[16] == 1 and not p[17:16 + 882].any() and p[-1] == 9
    p = R.pack(FRAMES["last"][None])
    assert p[16 + 881] == 0x80 and not p[16:16 + 881].any() and p[-1] == 200
    p = R.pack(FRAMES["group"][None])
    assert p[16 + 10] == 0xFF and p[16 + 11] == 0xFF and p[16:16 + 882].sum() == 2 * 255
    assert p[16 + 882:].tolist() == list(range(1, 17))
    p = R.pack(FRAMES["zero"][None])
    assert p.size == 8 + 8 + 882 and struct.unpack("<II", p[:8].tobytes()) == (1, 0) and not p[8:].any()
    p = R.pack(FRAMES["full"][None])
    assert p.size == 16 + 882 + FB and (p[16:16 + 882] == 0xFF).all() and struct.unpack("<H", p[8:10].tobytes()) == (FB,)


def test_chunks_and_formula():
    order = ["sparse", "zero", "full", "first", "last", "group", "dense"]
    f = np.stack([FRAMES[k] for k in order])
    one = R.pack(f)                       # one chunk of 7
    assert one.tobytes() == _pack_by_definition(list(f))
    assert one.size == R.packed_size(f) == 8 + 16 + 7 * 882 + int(np.count_nonzero(f))
    three = R.pack(f, chunk_frames=3)     # chunks of 3, 3, 1
    assert three.tobytes() == b"".join(_pack_by_definition(list(f[i:i + 3])) for i in (0, 3, 6))
    assert three.size == R.packed_size(f, 3) == 3 * 8 + 8 + 8 + 8 + 7 * 882 + int(np.count_nonzero(f))
    assert np.array_equal(R.unpack(three, 7, 3), f) and np.array_equal(R.unpack(one, 7), f)
    # the worst case the staging is sized for: 7,938 B per frame
    assert R.packed_size(FRAMES["full"][None]) - 16 == 7938


def test_checksum_sees_order_and_single_bytes():
    f = np.stack([FRAMES["sparse"], FRAMES["dense"]])
    s = R.frame_checksum(f)
    # a sum over (word, position) pairs: the parts add up whatever the order they are computed in
    assert (R.frame_checksum(f[:1], 0) + R.frame_checksum(f[1:], 1)) % 2**64 == s
    assert R.frame_checksum(f[::-1]) != s
    g = f.copy(); g[1, 4000] ^= 0x80
    assert R.frame_checksum(g) != s
    word = struct.unpack("<Q", f[0, 8:16].tobytes())[0]
    direct = sum(struct.unpack("<Q", f[0, 8 * k:8 * k + 8].tobytes())[0] * ((2 * k + 1) * R.CHECKSUM_MUL) for k in range(882))
    assert direct % 2**64 == R.frame_checksum(f[:1]) and word >= 0
