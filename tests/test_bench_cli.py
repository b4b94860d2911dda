"""bench.py's command line and output dump without a GPU: --full is off by default, and the dump of a stub learner is
float32 / float64, stays under its byte limit by a fixed seeded sample, and is the same from call to call."""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
import qlx


def _parse(argv, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_full_and_dump_are_off_by_default(monkeypatch):
    a = _parse(["--gpus", "1", "--steps", "7", "--warmup", "3"], monkeypatch)
    assert a.full is False and a.dump_outputs is None and (a.gpus, a.steps, a.warmup) == (1, 7, 3)
    a = _parse(["--full", "--dump-outputs", "some/dir"], monkeypatch)
    assert a.full is True and a.dump_outputs == "some/dir"


class _StubLearner:
    """qlx.SelfDrivingQLearner's read-out surface with fixed contents; U x B sampled indices / targets per step"""

    def __init__(self, n_envs, updates, batch):
        self.n, self.u, self.b = n_envs, updates, batch
        rng = np.random.default_rng(1)
        self._idx = rng.integers(0, 1 << 40, (updates, batch), dtype=np.uint64)
        self._tg = rng.standard_normal((updates, batch)).astype(np.float32)
        self.model = types.SimpleNamespace(get=lambda v: np.full(qlx.VAR_SHAPES[v], v + 0.5, np.float32))
        self.environment = types.SimpleNamespace(mechanics=self._mech, state=self._state)

    def last(self, max_updates=4096):
        z =np.zeros(self.n, np.uint8)
        return dict(actions=z + 2, rewards=z.astype(np.float32), dones=z, losses=np.ones(self.u, np.float32),
                    indices=self._idx, targets=self._tg)

    def _mech(self):
        m = np.zeros(self.n, qlx.STATE_DTYPE)
        m["score"] = np.arange(self.n)
        m["bricks"] = np.uint64(0xFFFF_FFFE_0000_0003)
        return m

    def _state(self):
        return (np.arange(self.n, dtype=np.uint8)[:, None, None, None] + np.zeros((1, 84, 84, 4), np.uint8))

    def stats(self):
        return {k: i for i, k in enumerate(bench.DUMP_STATS)}


def _dump(tmp_path, name, n_envs, updates, batch):
    run = object.__new__(bench.Run)
    run.L, run.ua, run.precision = _StubLearner(n_envs, updates, batch), max(1, n_envs // updates), "fp32"
    run.args, run.ctl = types.SimpleNamespace(envs=n_envs), types.SimpleNamespace(rank=0)
    run._dump(str(tmp_path / name))
    return {f[:-4]: np.load(tmp_path / name / f) for f in sorted(os.listdir(tmp_path / name))}


def test_dump_of_a_small_step_is_whole(tmp_path):
    d = _dump(tmp_path, "a", 128, 16, 32)
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    assert d["last_indices"].shape == (16, 32) and d["last_indices"].dtype == np.float64   # 2^40 does not fit float32
    assert np.array_equal(d["last_indices"], _StubLearner(128, 16, 32)._idx.astype(np.float64))
    assert d["last_actions"].tolist() == [2.0] * 128 and d["stats"].tolist() == list(range(8))
    # STATE_DTYPE's fields in order, bricks as its low and high halves
    names = [k for k in qlx.STATE_DTYPE.names if k != "bricks"]
    assert d["env_mechanics"].shape == (128, len(names) + 2)
    assert np.array_equal(d["env_mechanics"][:, names.index("score")], np.arange(128))
    assert (d["env_mechanics"][:, -2] == 3.0).all() and (d["env_mechanics"][:, -1] == float(0xFFFF_FFFE)).all()
    # the acting frames of 64 distinct envs, named beside them
    envs = d["acting_frames_envs"].astype(int)
    assert len(set(envs.tolist())) == 64 and (np.diff(envs) > 0).all() and envs.max() < 128
    assert d["acting_frames"].shape == (64, 84, 84, 4) and np.array_equal(d["acting_frames"][:, 0, 0, 0], envs)
    assert d["online_6_full_layer_kernel"].shape == (3136, 512) and (d["online_6_full_layer_kernel"] == 6.5).all()


def test_dump_stays_under_its_limit_and_repeats(tmp_path):
    """10 M sampled indices (80 MB as float64) and targets (40 MB): cut to a fixed seeded sample in index order."""
    a = _dump(tmp_path, "a", 64, 10_000, 1_000)
    b = _dump(tmp_path, "b", 64, 10_000, 1_000)
    assert sum(x.nbytes for x in a.values()) <= bench.DUMP_MAX_BYTES == 64_000_000
    assert a["last_indices"].ndim == 1 and a["last_indices"].size < 10_000_000
    assert a["online_6_full_layer_kernel"].shape == (3136, 512)   # what fits is left whole
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
