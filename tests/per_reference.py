"""Numpy restatement of the replay's prioritized calls (include/qlx.h "Prioritized replay on device tensors", DESIGN.md
§17): what the leaves, per_max and the tree are after any sequence of enables, pushes and priority writes, and the
logical <-> physical index mapping.  The power is the build's own (oracle.det_powf), the draws are the oracle sampler's
(oracle.per_sample) over these leaves; nothing here has a tolerance."""
import numpy as np

import oracle as O


def leaves_pow2(cap):
    L = 1
    while L < cap:
        L <<= 1
    return L


def build_tree(leaves):
    """the heap [2L] over `leaves` [cap]: node i = t[2i] + t[2i + 1], one fp32 add each, level by level"""
    leaves = np.asarray(leaves, np.float32)
    L = leaves_pow2(leaves.shape[0])
    t = np.zeros(2 * L, np.float32)
    t[L:L + leaves.shape[0]] = leaves
    w = L >> 1
    while w >= 1:
        t[w:2 * w] = t[2 * w:4 * w:2] + t[2 * w + 1:4 * w:2]
        w >>= 1
    return t


class PerRef:
    """the priorities of a ring of `cap` slots that has had `total` pushes when priorities are enabled"""

    def __init__(self, cap, total=0):
        self.cap = cap
        self.total = total
        self.leaves = np.zeros(cap, np.float32)
        self.leaves[:self.len] = 1.0
        self.per_max = np.float32(1.0)

    @property
    def len(self):
        return min(self.total, self.cap)

    @property
    def start(self):
        """physical slot of logical index 0 (the oldest transition)"""
        return (self.total - self.len) % self.cap

    def to_physical(self, idx):
        return (np.asarray(idx).astype(np.uint64) + np.uint64(self.start)) % np.uint64(self.cap)

    def to_logical(self, slots):
        return (np.asarray(slots).astype(np.uint64) + np.uint64(self.cap - self.start)) % np.uint64(self.cap)

    def push(self, n):
        """n new transitions enter at per_max"""
        for e in range(n):
            self.leaves[(self.total + e) % self.cap] = self.per_max
        self.total += n

    def update(self, indices, td_abs, alpha=0.6, eps=1e-6):
        """Guarded last-writer-wins priority write; returns whether any entry was refused (the sticky flag).  An int64
        index is read as the ABI's uint64, so a negative one is >= len."""
        idx = np.asarray(indices).astype(np.int64).view(np.uint64)
        td = np.asarray(td_abs, np.float32)
        with np.errstate(invalid="ignore"):
            ok = (idx < np.uint64(self.len)) & (td >= 0) & np.isfinite(td)
        pr = O.det_powf(np.where(ok, td, np.float32(0)) + np.float32(eps), alpha)
        slots = (np.where(ok, idx, np.uint64(0)) + np.uint64(self.start)) % np.uint64(self.cap)
        for k in np.flatnonzero(ok):
            self.leaves[slots[k]] = pr[k]
        if ok.any():
            self.per_max = max(self.per_max, pr[ok].max())
        return not ok.all()

    def tree(self):
        return build_tree(self.leaves)

    def sample(self, seed, update_idx, rank, beta, batch):
        """(logical indices uint64 [batch], weights float32 [batch], total) of one batch"""
        slots, w, total = O.per_sample(self.leaves, seed, update_idx, 1, rank, self.len, beta, batch)
        return self.to_logical(slots[0]), w[0], np.float32(total)
