"""Learner and replay snapshots on the GPU (qlx_learner_save / _load, qlx_replay_save / _load): a learner that is saved,
closed and loaded again continues bit for bit like one that never stopped - every output of every following vector step,
and at the end the envs, both models, the replay, the prioritized-replay leaves, the episode books and the statistics.
Also: two saves of one state are byte-identical, the info block, the RAW codec arm (QLX_SNAPSHOT_PACK=0), the replay
alone, corrupted files (status -6, nothing created, no memory lost) and that saving does not disturb a learner."""
import os
import subprocess
import sys

import numpy as np
import pytest

import snapshot_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S2 = 12


def _qlx():
    import qlx
    return qlx


@pytest.fixture(scope="module", autouse=True)
def torch_device_ready():
    """torch's own device context (test_failed_loads_leak_nothing reads free memory through it) is opened before any test of this module
    starts a child process: opened afterwards, it has been seen to find no device"""
    import torch
    torch.cuda.mem_get_info()


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def base_params(**kw):
    """the ring wraps (96 < 8 x 20), greedy acting is on from the third vector step, a statistics event every 8 steps"""
    p = dict(n_envs=8, batch_size=16, history_buffer_len=96, max_steps_per_episode=45, update_after_actions=8,
             epsilon_pure_random_steps=16, epsilon_max=0.5, epsilon_min=0.05, epsilon_greedy_steps=400.0,
             stats_after_steps=64, episode_reward_history_buffer_len=5)
    p.update(kw)
    return p


def configs():
    qlx = _qlx()
    return {
        "f32_memo": dict(),
        "f32_ddqn_per_sync": dict(flags=qlx.DOUBLE_DQN | qlx.PER, target_sync_steps=40),
        "f32_nstep3": dict(n_step=3),
        "bf16_memo": dict(qnet_precision=qlx.PREC_BF16),
        # episodes cut without a done before and after the save point (the n-step windows end at the cuts)
        "f32_nstep3_short_episodes": dict(n_step=3, max_steps_per_episode=7),
    }


CASES = [(name, s1) for name in ("f32_memo", "f32_ddqn_per_sync", "f32_nstep3", "bf16_memo", "f32_nstep3_short_episodes")
         for s1 in (20, 5)]


def full_state(L, per):
    """everything comparable of a learner between vector steps"""
    n = len(L.replay_buffer)
    idx = np.arange(n, dtype=np.uint64)
    out = dict(hashes=L.environment.hashes(), mechanics=L.environment.mechanics(), obs=L.environment.state(),
               stats=L.stats(), episode_rewards=L.episode_rewards(), action_counts=L.action_counts(),
               stats_events=L.stats_events(), last_log=L.last_log())
    out["log"] = L.learning_update_log() if len(out["episode_rewards"]) else ""
    for name, m in (("online", L.model), ("target", L.stabilized_model)):
        out[name + "_iterations"] = m.iterations()
        for var in range(10):
            for which in range(3):
                out["%s_%d_%d" % (name, var, which)] = m.get(var, which)
    for k, v in L.replay_buffer.get_many(idx).items():
        out["replay_" + k] = v
    for k, v in L.replay_buffer.nstep(idx, 3, 0.99).items():
        out["nstep_" + k] = v
    if per:
        _, leaves, pmax = L.priorities()
        out["per_leaves"], out["per_max"] = leaves, pmax
    return out


def assert_same_state(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert same(a[k], b[k]), k
        elif isinstance(a[k], dict):
            assert {x: repr(y) for x, y in a[k].items()} == {x: repr(y) for x, y in b[k].items()}, k   # (NaN-proof)
        else:
            assert a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]), k


def step_both(a, b, steps):
    updates = 0
    for v in range(steps):
        a.vector_step()
        b.vector_step()
        la, lb = a.last(), b.last()
        for k in ("actions", "rewards", "dones", "losses", "indices", "targets"):
            assert same(la[k], lb[k]), (k, v)
        updates += len(la["losses"])
    return updates


@pytest.mark.parametrize("name, s1", CASES, ids=["%s-S1_%d" % c for c in CASES])
def test_resume_is_exact(name, s1, tmp_path):
    qlx = _qlx()
    kw = base_params(**configs()[name])
    per = bool(kw.get("flags", 0) & qlx.PER)
    path = tmp_path / "learner.qlx"
    a = qlx.SelfDrivingQLearner(qlx.Parameter(**kw))
    b = qlx.SelfDrivingQLearner(qlx.Parameter(**kw))
    try:
        a.run(s1)
        b.run(s1)
        b.save(path)
        b.close()
        b = qlx.SelfDrivingQLearner.load(path)
        assert len(b.last()["losses"]) == 0     # the last step's outputs are not part of a snapshot
        assert bytes(b.param) == bytes(a.param)
        assert len(b.replay_buffer) == min(8 * s1, 96)
        assert step_both(a, b, S2) == S2        # one update per vector step, on both sides of the save point
        sa, sb = full_state(a, per), full_state(b, per)
        assert_same_state(sa, sb)
        assert sa["stats"]["step_count"] == 8 * (s1 + S2) and sa["stats"]["update_count"] > S2
        if kw["max_steps_per_episode"] == 7:
            assert sa["stats"]["episode_count"] >= 8 * ((s1 + S2) // 7) and len(sa["episode_rewards"]) == 5
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("saver, loader", [("1", "0"), ("0", "1")], ids=["memo_ignored", "memo_rebuilt"])
def test_resume_across_the_memo_switch(saver, loader, tmp_path, monkeypatch):
    """QLX_TARGET_CACHE is read when a learner is created, also by a load: a process without the memo ignores the file's,
    and one that wants a memo the file does not hold rebuilds it at its first push - the same run either way (the memo
    and the per-batch target pass give the same values, test_gpu_learner)"""
    qlx = _qlx()
    kw = base_params()
    path = tmp_path / "learner.qlx"
    monkeypatch.delenv("QLX_TARGET_CACHE", raising=False)
    a = qlx.SelfDrivingQLearner(qlx.Parameter(**kw))
    monkeypatch.setenv("QLX_TARGET_CACHE", saver)
    b = qlx.SelfDrivingQLearner(qlx.Parameter(**kw))
    try:
        a.run(20)
        b.run(20)
        b.save(path)
        b.close()
        assert (R.SEC_MEMO in R.read_container(path)["sections"]) == (saver == "1")
        monkeypatch.setenv("QLX_TARGET_CACHE", loader)
        b = qlx.SelfDrivingQLearner.load(path)
        assert step_both(a, b, S2) == S2
        assert_same_state(full_state(a, False), full_state(b, False))
    finally:
        a.close()
        b.close()


def test_saves_are_deterministic_and_info(tmp_path, monkeypatch):
    qlx = _qlx()
    monkeypatch.delenv("QLX_SNAPSHOT_PACK", raising=False)
    kw = base_params(flags=qlx.PER, learner_seed=77)
    L = qlx.SelfDrivingQLearner(qlx.Parameter(**kw))
    try:
        L.run(20)
        p1, p2, p3 = tmp_path / "a.qlx", tmp_path / "b.qlx", tmp_path / "raw.qlx"
        L.save(p1)
        L.save(p2)
        monkeypatch.setenv("QLX_SNAPSHOT_PACK", "0")    # read at every save
        L.save(p3)
        monkeypatch.delenv("QLX_SNAPSHOT_PACK")
        st = L.stats()
    finally:
        L.close()
    assert p1.read_bytes() == p2.read_bytes()
    assert not list(tmp_path.glob("*.tmp"))
    info, raw = qlx.snapshot_info(p1), qlx.snapshot_info(p3)
    for i, p in ((info, p1), (raw, p3)):
        assert (i["format_version"], i["kind"], i["reserved"]) == (1, qlx.SNAPSHOT_LEARNER, 0)
        for k in ("step_count", "vec_steps", "update_count", "episode_count", "replay_len"):
            assert i[k] == st[k], k
        assert i["replay_total"] == 160 and i["file_bytes"] == p.stat().st_size
        assert bytes(i["params"]) == bytes(qlx.Parameter(**kw))
        # the env's 4 ring frames per env + the replay's live frames: min(total, capacity + 4 n_envs)
        assert i["frames"] == 32 + 128 and i["frame_bytes_raw"] == 160 * 7056
    assert info["frame_codec"] == qlx.FRAME_CODEC_BITMAP and raw["frame_codec"] == qlx.FRAME_CODEC_RAW
    assert info["frame_bytes_stored"] < 0.5 * info["frame_bytes_raw"]   # Breakout frames: about 0.225
    assert raw["frame_bytes_stored"] == raw["frame_bytes_raw"]
    # the file's own structure, as tests/snapshot_reference.py restates it
    c = R.read_container(p1)
    assert c["magic"] == b"QLXSNAP1" and c["file_bytes"] == c["size"]
    assert set(c["sections"]) == {R.SEC_INFO, R.SEC_LEARNER, R.SEC_ENV, R.SEC_ENV_FRAMES, R.SEC_REPLAY, R.SEC_REPLAY_FRAMES,
                                  R.SEC_MODEL_ONLINE, R.SEC_MODEL_TARGET, R.SEC_BOOKS, R.SEC_PER, R.SEC_MEMO}
    fs = R.frame_section(p1, R.SEC_REPLAY_FRAMES)
    assert (fs["codec"], fs["chunk_frames"], fs["n_frames"]) == (1, R.CHUNK_FRAMES, 128)
    # the raw file's frames pack, by the numpy restatement, into exactly the payload of the packed file
    fr = R.frame_section(p3, R.SEC_REPLAY_FRAMES)
    blob = p3.read_bytes()
    frames = np.frombuffer(blob[fr["payload"]:fr["payload"] + 128 * 7056], np.uint8).reshape(128, 7056)
    assert R.frame_checksum(frames) == fr["checksum"] == fs["checksum"]
    assert R.pack(frames).tobytes() == p1.read_bytes()[fs["payload"]:fs["payload"] + fs["stored_bytes"]]


_CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
import qlx
kw = eval(sys.argv[3])
L = qlx.SelfDrivingQLearner(qlx.Parameter(**kw))
L.run(int(sys.argv[4]))
L.save(sys.argv[2])
L.close()
"""


def test_raw_codec_resumes_exactly(tmp_path):
    """the A/B arm and fallback: a child process with QLX_SNAPSHOT_PACK=0 runs S1 steps and saves; this process loads the
    file and continues like a learner that never stopped"""
    qlx = _qlx()
    kw = base_params()
    path = tmp_path / "raw.qlx"
    env = dict(os.environ, QLX_SNAPSHOT_PACK="0")
    r = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(ROOT, "q-learning_amd"), str(path), repr(kw), "20"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert qlx.snapshot_info(path)["frame_codec"] == qlx.FRAME_CODEC_RAW
    a = qlx.SelfDrivingQLearner(qlx.Parameter(**kw))
    b = None
    try:
        a.run(20)
        b = qlx.SelfDrivingQLearner.load(path)
        assert step_both(a, b, S2) == S2
        assert_same_state(full_state(a, False), full_state(b, False))
    finally:
        a.close()
        if b is not None:
            b.close()


@pytest.mark.parametrize("steps", [15, 7, 0], ids=["wrapped", "part_filled", "empty"])
def test_replay_alone(steps, tmp_path):
    qlx = _qlx()
    n, cap = 4, 40
    env = qlx.BreakoutEnvironment(n, seed=3)
    rb = qlx.ReplayBuffer(cap, n)
    rng = np.random.default_rng(steps)
    path = tmp_path / "replay.qlx"
    rb2 = None
    try:
        for t in range(steps):
            a = rng.integers(0, 3, n)
            _, r, d = env.step(a)
            rb.add(env, a, r, d)
            if t == 9:
                env.reset([1, 0, 1, 0])
        rb.save(path)
        info = qlx.snapshot_info(path)
        assert (info["kind"], info["replay_total"], info["replay_len"]) == (qlx.SNAPSHOT_REPLAY, n * steps, min(n * steps, cap))
        assert info["frames"] == min(n * steps, cap + 4 * n)
        assert (info["params"].n_envs, info["params"].history_buffer_len, info["params"].batch_size) == (n, cap, 0)
        rb2 = qlx.ReplayBuffer.load(path)
        assert len(rb2) == len(rb) == min(n * steps, cap)
        if steps:
            idx = np.arange(len(rb), dtype=np.uint64)
            g1, g2 = rb.get_many(idx), rb2.get_many(idx)
            for k in g1:
                assert same(g1[k], g2[k]), k
            assert g1["state_next"].any()
            assert same(rb.sample_distinct(5, 3, 16), rb2.sample_distinct(5, 3, 16))
            w1, w2 = rb.nstep(idx, 3, 0.9), rb2.nstep(idx, 3, 0.9)
            for k in w1:
                assert same(w1[k], w2[k]), k
        with pytest.raises(qlx.QlError, match="status -6"):   # a replay file is no learner file
            qlx.SelfDrivingQLearner.load(path)
    finally:
        env.close()
        rb.close()
        if rb2 is not None:
            rb2.close()


@pytest.fixture(scope="module")
def bad_files(tmp_path_factory):
    """a good learner snapshot and four corrupted copies: {name: (path, what the error names)}"""
    qlx = _qlx()
    tmp = tmp_path_factory.mktemp("bad_files")
    L = qlx.SelfDrivingQLearner(qlx.Parameter(**base_params()))
    good = tmp / "good.qlx"
    try:
        L.run(14)
        L.save(good)
    finally:
        L.close()
    blob = good.read_bytes()
    fs = R.frame_section(good, R.SEC_REPLAY_FRAMES)
    assert fs["codec"] == 1 and fs["value_bytes"] > 100

    def corrupt(name, offset):
        b = bytearray(blob)
        b[offset] ^= 0x10
        p = tmp / name
        p.write_bytes(bytes(b))
        return p

    truncated = tmp / "truncated.qlx"
    truncated.write_bytes(blob[:len(blob) * 2 // 3])
    return dict(
        good=(good, None),
        truncated=(truncated, "short file"),
        # 0x10 flipped in a value byte ({255, 236, ...}: still non-zero): only the device checksum sees it
        value=(corrupt("value.qlx", fs["values_offset"] + 57), "frame checksum"),
        # a mask bit: refused by the host validator before any launch
        mask=(corrupt("mask.qlx", fs["mask_offset"] + 3 * 882 + 400), "disagrees with its mask"),
        small=(corrupt("small.qlx", R.read_container(good)["sections"][R.SEC_MODEL_TARGET][0] + 12345),
               "checksum mismatch in section"))


def test_bad_files_are_refused(bad_files, tmp_path):
    qlx = _qlx()
    for name in ("truncated", "value", "mask", "small"):
        p, needle = bad_files[name]
        with pytest.raises(qlx.QlError, match="status -6") as ei:
            qlx.SelfDrivingQLearner.load(p)
        assert needle in str(ei.value), str(ei.value)
    good = bad_files["good"][0]
    with pytest.raises(qlx.QlError, match="status -6"):
        qlx.ReplayBuffer.load(good)                                  # wrong kind
    with pytest.raises(qlx.QlError, match="status -6"):
        qlx.SelfDrivingQLearner.load(tmp_path / "missing.qlx")
    ok = qlx.SelfDrivingQLearner.load(good)                          # the good file still loads
    ok.close()


def test_failed_loads_leak_nothing(bad_files):
    """the learner is built before the frames are read: a failed load gives everything back (the 64 MB of allocator slack
    are test_invalid_parameters_fail_loudly's)"""
    import torch
    qlx = _qlx()
    free0 = torch.cuda.mem_get_info()[0]
    for i in range(20):
        with pytest.raises(qlx.QlError, match="status -6"):
            qlx.SelfDrivingQLearner.load(bad_files[("value", "mask", "truncated", "small")[i % 4]][0])
    assert torch.cuda.mem_get_info()[0] >= free0 - (64 << 20)


def test_saving_does_not_disturb_the_learner(tmp_path):
    qlx = _qlx()
    kw = base_params(flags=qlx.PER)
    a = qlx.SelfDrivingQLearner(qlx.Parameter(**kw))
    b = qlx.SelfDrivingQLearner(qlx.Parameter(**kw))
    try:
        a.run(6)
        b.run(6)
        for v in range(4):
            a.save(tmp_path / ("step%d.qlx" % v))
            assert step_both(a, b, 1) == 1
            assert same(a.environment.hashes(), b.environment.hashes())
            assert same(a.environment.mechanics(), b.environment.mechanics())
            assert a.stats() == b.stats()
        assert_same_state(full_state(a, True), full_state(b, True))
    finally:
        a.close()
        b.close()
