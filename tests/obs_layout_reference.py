"""Numpy restatement of the NCHW_TIME state layout (include/qlx.h) from the NHWC_SLOT bytes.

NHWC_SLOT is the reference tensor view [n][x][y][ring slot]; the frame of episode step m sits in ring slot (m - 1) & 3,
so the oldest of the four frames is the one the next step will overwrite.  NCHW_TIME [n][age][x][y] lists them oldest
first: channel c is ring slot (first + c) & 3 with
    first = next_slot       for an env (next_slot = steps taken & 3),
    first = k & 3           for s' of a replay transition of episode step k,
    first = (k - 1) & 3     for its s.
Frames the episode does not have yet are zero in the ring itself, so nothing else is needed.
"""
import numpy as np


def nchw_time(nhwc_slot, first):
    """[n][84][84][4] (x, y, slot) and the first slot per sample -> [n][4][84][84] (age, x, y)"""
    x = np.asarray(nhwc_slot)
    first = np.broadcast_to(np.asarray(first, dtype=np.int64), (x.shape[0],))
    out = np.empty((x.shape[0], 4) + x.shape[1:3], x.dtype)
    for c in range(4):
        slot = (first + c) & 3
        out[:, c] = np.take_along_axis(x, slot[:, None, None, None], axis=3)[..., 0]
    return out


def env_nchw_time(nhwc_slot, next_slot):
    return nchw_time(nhwc_slot, next_slot)


def replay_nchw_time(nhwc_slot, epstep, s_next):
    """states of replay transitions of episode step `epstep` (1-based): s' if s_next else s"""
    k = np.asarray(epstep, dtype=np.int64)
    return nchw_time(nhwc_slot, k if s_next else k - 1)
