"""numpy restatement of the snapshot frame codec QLX_FRAME_CODEC_BITMAP and of the snapshot container's layout
(q-learning_amd/csrc/snapshot_format.h), for the tests of the GPU codec and of the files the library writes.

A frame is 7,056 bytes.  Packed frame: a mask of 882 bytes (bit i & 7 of byte i >> 3 set iff byte i is non-zero) and the
non-zero bytes in ascending i.  A chunk of n <= C frames: {u32 n_frames, u32 value_bytes}, u16 nnz[n] zero-padded to 8
bytes, the masks [n][882], the values of all frames in frame order.  A packed stream is its chunks, every one but the
last holding C frames.
"""
import struct

import numpy as np

FRAME_BYTES = 7056
MASK_BYTES = 882
CHUNK_FRAMES = 512          # C of the files and streams the library writes
CHECKSUM_MUL = 0x9E3779B97F4A7C15
DATA_START = 64 + 16 * 32   # file header + section table
SEC_INFO, SEC_LEARNER, SEC_ENV, SEC_ENV_FRAMES, SEC_REPLAY, SEC_REPLAY_FRAMES = 1, 2, 3, 4, 5, 6
SEC_MODEL_ONLINE, SEC_MODEL_TARGET, SEC_BOOKS, SEC_PER, SEC_MEMO = 7, 8, 9, 10, 11


def _pad8(x):
    return (x + 7) & ~7


def chunk_fixed_bytes(n):
    return 8 + _pad8(2 * n) + MASK_BYTES * n


def pack_chunk(frames):
    f = np.ascontiguousarray(frames, np.uint8).reshape(-1, FRAME_BYTES)
    n = f.shape[0]
    nz = f != 0
    nnz = nz.sum(axis=1).astype("<u2")
    values = f[nz]                                             # row-major: frame order, ascending byte index
    masks = np.packbits(nz, axis=1, bitorder="little")         # [n][882]
    head = np.zeros(8 + _pad8(2 * n), np.uint8)
    head[:8] = np.frombuffer(struct.pack("<II", n, values.size), np.uint8)
    head[8:8 + 2 * n] = nnz.view(np.uint8)
    return np.concatenate([head, masks.reshape(-1), values])


def pack(frames, chunk_frames=CHUNK_FRAMES):
    f = np.ascontiguousarray(frames, np.uint8).reshape(-1, FRAME_BYTES)
    return np.concatenate([pack_chunk(f[i:i + chunk_frames]) for i in range(0, f.shape[0], chunk_frames)])


def packed_size(frames, chunk_frames=CHUNK_FRAMES):
    """the formula: 882 + nnz bytes per frame, plus each chunk's header and nnz table"""
    f = np.ascontiguousarray(frames, np.uint8).reshape(-1, FRAME_BYTES)
    n = f.shape[0]
    per_frame = MASK_BYTES * n + int(np.count_nonzero(f))
    tables = sum(8 + _pad8(2 * min(chunk_frames, n - i)) for i in range(0, n, chunk_frames))
    return per_frame + tables


def unpack(packed, n_frames, chunk_frames=CHUNK_FRAMES):
    p = np.ascontiguousarray(packed, np.uint8)
    out = np.zeros((n_frames, FRAME_BYTES), np.uint8)
    at = done = 0
    while done < n_frames:
        n, vb = struct.unpack("<II", p[at:at + 8].tobytes())
        assert n == min(chunk_frames, n_frames - done)
        fixed = chunk_fixed_bytes(n)
        nnz = p[at + 8:at + 8 + 2 * n].view("<u2")
        masks = p[at + 8 + _pad8(2 * n):at + fixed].reshape(n, MASK_BYTES)
        nz = np.unpackbits(masks, axis=1, bitorder="little").astype(bool)
        assert np.array_equal(nz.sum(axis=1), nnz) and int(nnz.sum()) == vb
        out[done:done + n][nz] = p[at + fixed:at + fixed + vb]
        at += fixed + vb
        done += n
    assert at == p.size
    return out


def frame_checksum(frames, first=0):
    """sum over the frames' 8-byte words w_j (j = frame ordinal * 882 + word) of w_j * ((2 j + 1) * kH1), mod 2^64"""
    w = np.ascontiguousarray(frames, np.uint8).reshape(-1).view("<u8")
    j = np.arange(w.size, dtype=np.uint64) + np.uint64(first * 882)
    with np.errstate(over="ignore"):
        mul = (j * np.uint64(2) + np.uint64(1)) * np.uint64(CHECKSUM_MUL)
        return int((w * mul).sum(dtype=np.uint64))


def read_container(path):
    """header fields and {section id: (offset, bytes, checksum)} of a snapshot file"""
    raw = open(path, "rb").read()
    magic, version, kind, n_sections, crc, file_bytes = struct.unpack("<8sIIIIQ", raw[:32])
    sections = {}
    for i in range(n_sections):
        sid, _, off, size, cks = struct.unpack("<IIQQQ", raw[64 + 32 * i:96 + 32 * i])
        sections[sid] = (off, size, cks)
    return dict(magic=magic, version=version, kind=kind, file_bytes=file_bytes, size=len(raw), sections=sections)


def frame_section(path, sid):
    """a frame section's header and where its parts lie in the file: codec, chunk_frames, n_frames, payload offset,
    and for the bitmap codec the (mask offset, values offset, value_bytes) of its first chunk"""
    c = read_container(path)
    off, size, cks = c["sections"][sid]
    raw = open(path, "rb").read()
    codec, chunk_frames, n_frames, raw_bytes, stored = struct.unpack("<IIQQQ", raw[off:off + 32])
    out = dict(codec=codec, chunk_frames=chunk_frames, n_frames=n_frames, raw_bytes=raw_bytes, stored_bytes=stored,
               payload=off + 32, checksum=cks)
    if codec == 1 and n_frames:
        n, vb = struct.unpack("<II", raw[off + 32:off + 40])
        out.update(first_chunk_frames=n, mask_offset=off + 32 + 8 + _pad8(2 * n),
                   values_offset=off + 32 + chunk_fixed_bytes(n), value_bytes=vb)
    return out
