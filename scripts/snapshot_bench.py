#!/usr/bin/env python3
"""A/B measurement of the snapshot frame codec (DESIGN.md "Snapshots").

Shape: config C3's replay - 8,192 envs, a replay of 1,000,000 transitions filled by qlx_learner_prefill (random acting,
no updates), B = 1024 - so a snapshot holds 1,032,768 replay frames + 32,768 env ring frames of 7,056 B.  The two arms
are the frame codecs: QLX_FRAME_CODEC_BITMAP (the default) and QLX_FRAME_CODEC_RAW (QLX_SNAPSHOT_PACK=0, read at every
save; a load takes the codec from the file).  One process; after a warm-up save + load per arm, `pairs` rounds of
(bitmap save, raw save, bitmap load, raw load), each timed with a host clock around the synchronising call.  The codec
kernels' own time comes from HIP events around every chunk's kernels (QLX_SNAPSHOT_TIMING=<file>: the library appends one
JSON line per save / load with the summed kernel time and the bytes those kernels read and wrote).  One JSON line per
arm with every wall time, and a summary line with median [min..max] and whether the ranges of save + load are separate;
nothing is asserted.

  python scripts/snapshot_bench.py [--pairs 5] [--envs 8192] [--replay 1000000] [--batch 1024] [--dir DIR] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "q-learning_amd"))
import qlx  # noqa: E402

ARMS = {"bitmap": None, "raw": "0"}   # QLX_SNAPSHOT_PACK


def timed_save(learner, path, arm):
    if ARMS[arm] is None:
        os.environ.pop("QLX_SNAPSHOT_PACK", None)
    else:
        os.environ["QLX_SNAPSHOT_PACK"] = ARMS[arm]
    try:
        t0 = time.perf_counter()
        learner.save(path)
        return time.perf_counter() - t0
    finally:
        os.environ.pop("QLX_SNAPSHOT_PACK", None)


def timed_load(path):
    t0 = time.perf_counter()
    learner = qlx.SelfDrivingQLearner.load(path)
    dt = time.perf_counter() - t0
    learner.close()
    return dt


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--replay", type=int, default=1_000_000)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--dir", default=None, help="directory the snapshots are written to (default: a temporary one)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sink = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    tmp = tempfile.TemporaryDirectory(dir=args.dir)
    timing = os.path.join(tmp.name, "timing.jsonl")
    os.environ["QLX_SNAPSHOT_TIMING"] = timing
    paths = {arm: os.path.join(tmp.name, arm + ".qlx") for arm in ARMS}
    st = os.statvfs(tmp.name)
    emit(dict(kind="target", dir=tmp.name, free_bytes=st.f_bavail * st.f_frsize))

    learner = qlx.SelfDrivingQLearner(qlx.Parameter(n_envs=args.envs, batch_size=args.batch, history_buffer_len=args.replay,
                                                    stats_after_steps=0))
    steps = -(-args.replay // args.envs) + 4     # the ring full, the frame ring with it
    t0 = time.perf_counter()
    learner.prefill(steps)
    learner.sync()
    emit(dict(kind="prefill", vector_steps=steps, seconds=time.perf_counter() - t0, replay_len=len(learner.replay_buffer)))

    wall = {arm: dict(save_s=[], load_s=[]) for arm in ARMS}
    for arm in ARMS:                              # warm-up: code objects, pinned buffers, the page cache's first touch
        timed_save(learner, paths[arm], arm)
        timed_load(paths[arm])
    open(timing, "w").close()
    for _ in range(args.pairs):
        for arm in ARMS:
            wall[arm]["save_s"].append(timed_save(learner, paths[arm], arm))
        for arm in ARMS:
            wall[arm]["load_s"].append(timed_load(paths[arm]))
    learner.close()

    kernels = {arm: dict(pack_us=[], unpack_us=[], pack_hbm_bytes=[], unpack_hbm_bytes=[]) for arm in ARMS}
    for line in open(timing):
        rec = json.loads(line)
        arm = "bitmap" if rec["codec"] == qlx.FRAME_CODEC_BITMAP else "raw"
        side = "pack" if rec["op"].endswith("save") else "unpack"
        kernels[arm][side + "_us"].append(rec["kernel_us"])
        kernels[arm][side + "_hbm_bytes"].append(rec["kernel_hbm_bytes"])

    summary = dict(kind="summary", pairs=args.pairs)
    for arm in ARMS:
        info = qlx.snapshot_info(paths[arm])
        total = [s + l for s, l in zip(wall[arm]["save_s"], wall[arm]["load_s"])]
        rec = dict(kind="arm", arm=arm, file_bytes=info["file_bytes"], frames=info["frames"],
                   frame_bytes_raw=info["frame_bytes_raw"], frame_bytes_stored=info["frame_bytes_stored"],
                   save=spread(wall[arm]["save_s"]), load=spread(wall[arm]["load_s"]), save_plus_load=spread(total), **wall[arm])
        if arm == "bitmap":
            k = kernels[arm]
            rec.update(pack_kernels_us=spread(k["pack_us"]), unpack_kernels_us=spread(k["unpack_us"]),
                       pack_hbm_bytes=k["pack_hbm_bytes"][0], unpack_hbm_bytes=k["unpack_hbm_bytes"][0],
                       pack_tb_per_s=k["pack_hbm_bytes"][0] / statistics.median(k["pack_us"]) / 1e6,
                       unpack_tb_per_s=k["unpack_hbm_bytes"][0] / statistics.median(k["unpack_us"]) / 1e6)
        emit(rec)
        summary[arm] = rec["save_plus_load"]
        summary[arm + "_file_bytes"] = info["file_bytes"]
    b, r = summary["bitmap"], summary["raw"]
    summary["ranges_separate"] = b["max"] < r["min"] or r["max"] < b["min"]
    summary["faster"] = "bitmap" if b["median"] < r["median"] else "raw"
    emit(summary)
    tmp.cleanup()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
